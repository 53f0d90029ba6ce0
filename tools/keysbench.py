#!/usr/bin/env python3
"""The table's put and get by key against the record route at one rank: one process, HIP events on the launch
stream, the two routes of a case interleaved round by round, inputs rotating over several buffers so that no
timed call finds its inputs where the call before left them, medians; the two routes' results are compared
before anything is timed.

  python tools/keysbench.py [--keysizes 8,13,32] [--elemsizes 8,40] [--cases empty,present] [--n-m 16]
                            [--log2-capacity 25] [--sets 3] [--rounds 3] [--out profiles/table/keysbench_16M.jsonl]

The default is 16M keys into capacity 2^25 (load 0.5), as tools/addbench.py.  The inputs of a case are
`sets` buffers: the same 16M distinct keys in a different order each, with values of their own.  Cases:
  empty    a set into an emptied table (cleared outside the timed span): every key creates
  present  a set into the table that holds all its keys: nothing is created, every row is overwritten
The gets always find their keys: they read the table as the case's puts leave it.
Legs (one JSON line per keysize, elemsize and case; times are medians in ms):
  put_keys      DeviceTable.put_keys with status
  put_records   bucket_put_records(nranks=1) + put_records with status: the record route
  get_keys      DeviceTable.get_keys
  get_records   bucket_records(nranks=1) + get(head=8) + get_resolve: the record route
Every leg runs with preallocated outputs and workspaces, so a timed span holds kernels only.  Each route has
a table of its own, and both tables see the same calls in the same order.  The keys are splitmix64 outputs of
a counter in their first 8 bytes (a bijection: distinct) and more of the stream behind.
equal: status and counters of the two put routes, values and status of the two get routes, and the values
read back against the values put.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pdht_amd as P  # noqa: E402

SEED = 0x4B455953424E4348
M = 1 << 20


def progress(what):
    print(f"  .. {what}", file=sys.stderr, flush=True)


def stream_rows(n, nbytes, first, dev):
    """n rows of `nbytes` bytes of the splitmix64 stream from word `first` on; -> (rows, words used)."""
    w = (nbytes + 7) // 8
    words = P.splitmix64_fill(SEED, first, n * w, device=dev).view(n, w)
    return words.view(torch.uint8).view(n, 8 * w)[:, :nbytes].contiguous(), n * w


def case_legs(L, E, n, cap, case, nsets, dev):
    if L < 8:
        raise SystemExit("keysbench needs keys of >= 8 bytes (the distinct counter)")
    B = P.put_record_bytes(L, E) - 24
    base, used = stream_rows(n, L, 0, dev)
    keys = [base] + [base[torch.randperm(n, device=dev)] for _ in range(nsets - 1)]
    vals = []
    for _ in range(nsets):
        v, w = stream_rows(n, E, used, dev)
        vals.append(v)
        used += w
    tk, tr = P.DeviceTable(cap, B, dev), P.DeviceTable(cap, B, dev)  # one table per route
    ws = torch.empty(P.table_put_keys_workspace_bytes(n), dtype=torch.uint8, device=dev)
    bws = torch.empty(P.bucket_workspace_bytes(n, L, 1, records=True), dtype=torch.uint8, device=dev)
    st_k, st_r = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    prec = P.bucket_put_records(keys[0], vals[0], 1, workspace=bws)
    grec = P.bucket_records(keys[0], 1, workspace=bws)
    rep = torch.empty((n, 1 + B // 8), dtype=torch.int64, device=dev).view(torch.uint8).view(n, 8 + B)
    out_k, out_r = (torch.empty((n, E), dtype=torch.uint8, device=dev) for _ in range(2))
    gst_k, gst_r = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    present = case == "present"
    turn = {"put_keys": 0, "put_records": 0, "get_keys": 0, "get_records": 0}

    def prep(tab):
        if not present:
            tab.clear()

    def nxt(leg):
        turn[leg] = (turn[leg] + 1) % nsets
        return turn[leg]

    def put_keys():
        k = nxt("put_keys")
        tk.put_keys(keys[k], vals[k], status=st_k, workspace=ws)

    def put_records():
        k = nxt("put_records")
        P.bucket_put_records(keys[k], vals[k], 1, out=prec, workspace=bws)
        tr.put_records(prec[0], status=st_r, workspace=ws)

    def get_keys():
        k = nxt("get_keys")
        tk.get_keys(keys[k], E, values=out_k, status=gst_k)

    def get_records():
        k = nxt("get_records")
        P.bucket_records(keys[k], 1, out=grec, workspace=bws)
        tr.get(grec[0], head=8, out=rep)
        P.get_resolve(rep, keys[k], E, values=out_r, status=gst_r)

    def equal():
        ok = True
        for k in range(nsets):
            for leg in turn:
                turn[leg] = k - 1
            prep(tk), prep(tr)
            put_keys(), put_records()
            ok &= bool(torch.equal(st_k, st_r)) and int(st_k.count_nonzero()) == 0
            ok &= tk.counts()[:2] == tr.counts()[:2] == (n, 0)
            get_keys(), get_records()
            ok &= bool(torch.equal(out_k, out_r)) and bool(torch.equal(gst_k, gst_r))
            ok &= bool(torch.equal(out_k, vals[k])) and int(gst_k.count_nonzero()) == 0
        progress(f"equal: {ok}")
        return ok

    if present:
        for tab in (tk, tr):
            tab.put_keys(keys[0], vals[0], status=st_k, workspace=ws)
    legs = {
        "put_keys": (lambda: prep(tk), put_keys),
        "put_records": (lambda: prep(tr), put_records),
        "get_keys": (lambda: None, get_keys),
        "get_records": (lambda: None, get_records),
    }
    return legs, equal, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keysizes", default="8,13,32")
    ap.add_argument("--elemsizes", default="8,40")
    ap.add_argument("--cases", default="empty,present")
    ap.add_argument("--n-m", type=int, default=16, help="keys per batch, in units of 2^20")
    ap.add_argument("--log2-capacity", type=int, default=25)
    ap.add_argument("--sets", type=int, default=3, help="input buffers a leg rotates over")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, cap = a.n_m * M, 1 << a.log2_capacity
    path = a.out or os.path.join(ROOT, "profiles", "table", f"keysbench_{a.n_m}M.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for L in (int(x) for x in a.keysizes.split(",")):
            for E in (int(x) for x in a.elemsizes.split(",")):
                for case in a.cases.split(","):
                    progress(f"keysize {L} elemsize {E} {case}")
                    legs, equal, B = case_legs(L, E, n, cap, case, a.sets, dev)
                    ok = equal()  # (also the warm-up of every leg)
                    torch.cuda.synchronize()
                    ms = {k: [] for k in legs}
                    for _ in range(a.rounds):
                        for k, (prep, fn) in legs.items():  # the routes interleaved, leg by leg
                            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                                  for _ in range(a.sets)]
                            for s, e in ev:
                                prep()
                                s.record()
                                fn()
                                e.record()
                            torch.cuda.synchronize()
                            ms[k].extend(s.elapsed_time(e) for s, e in ev)
                            progress(f"{k}: {ms[k][-1]:.3f} ms")
                    med = {k: float(np.median(v)) for k, v in ms.items()}
                    row = {"keysize": L, "elemsize": E, "rowbytes": B, "case": case, "n": n, "capacity": cap,
                           "load": n / cap, "sets": a.sets, "equal": bool(ok),
                           "ms": {k: round(v, 4) for k, v in med.items()},
                           "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                           "Mkeys_s": {k: round(n / v / 1e3, 1) for k, v in med.items()},
                           "put_keys_vs_records": round(med["put_keys"] / med["put_records"], 3),
                           "get_keys_vs_records": round(med["get_keys"] / med["get_records"], 3),
                           "record_buffer_bytes": n * (24 + B)}
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                    del legs, equal
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
