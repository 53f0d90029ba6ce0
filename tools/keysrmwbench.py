#!/usr/bin/env python3
"""The table's update, insert-if-absent and compare-and-swap by key against their record routes at one rank
(and, for the swap, against the mbits route): tools/keysbench.py's method -- one process, HIP events on the
launch stream, the routes of an operation interleaved round by round, inputs rotating over several buffers,
medians; the routes' results are compared before anything is timed.

  python tools/keysrmwbench.py [--keysizes 8,13,32] [--elemsizes 8,40] [--cases empty,present] [--n-m 16]
                               [--log2-capacity 25] [--sets 3] [--rounds 3]
                               [--out profiles/table/keysrmwbench_16M.jsonl]

The default is 16M keys into capacity 2^25 (load 0.5).  The inputs are `sets` buffers: the same 16M distinct
keys in a different order each, with values of their own whose first word is 0.  Cases:
  empty    the table holds nothing: an update and a swap find no key, an add (into a table cleared outside the
           timed span) creates every key
  present  the table holds every key: an update overwrites every row, an add creates nothing, and every swap
           request swaps -- the word at the value's start goes 0 -> 1 in one call and 1 -> 0 in the next
Legs (one JSON line per keysize, elemsize and case; times are medians in ms):
  update_keys    DeviceTable.update_keys with status
  update_records bucket_put_records(nranks=1) + update_records with status
  add_keys       DeviceTable.add_keys with status
  add_records    bucket_put_records(nranks=1) + add_records with status
  cswap_keys     DeviceTable.cswap_keys
  cswap_records  bucket_records(nranks=1) + cswap on the records
  cswap_mbits    cswap on a dense mbits array that one put_keys(mbits=True) left: what a caller who keeps the
                 digests around pays (the hash is not in the span)
Every leg runs with preallocated outputs and workspaces, so a timed span holds kernels only.  Each route has a
table of its own, and the tables of an operation see the same calls in the same order.
equal: status and counters of the two update routes and of the two add routes, replies of the three swap
routes.
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

from keysbench import M, progress, stream_rows  # noqa: E402

OPS = ("update", "add", "cswap")


def op_legs(op, L, E, n, cap, case, nsets, dev):
    """-> ({leg: (prep, fn)}, equal) of one operation; its tables live as long as the closures."""
    if L < 8 or E < 8:
        raise SystemExit("keysrmwbench needs keys and values of >= 8 bytes (the distinct counter, the swapped word)")
    B = P.put_record_bytes(L, E) - 24
    slot = B - (E + 7) // 8 * 8
    base, used = stream_rows(n, L, 0, dev)
    keys = [base] + [base[torch.randperm(n, device=dev)] for _ in range(nsets - 1)]
    vals = []
    for _ in range(nsets):
        v, w = stream_rows(n, E, used, dev)
        v[:, :8] = 0
        vals.append(v)
        used += w
    present = case == "present"
    routes = ("keys", "records", "mbits") if op == "cswap" else ("keys", "records")
    tabs = {r: P.DeviceTable(cap, B, dev) for r in routes}
    ws = torch.empty(P.table_add_keys_workspace_bytes(n), dtype=torch.uint8, device=dev)
    bws = torch.empty(P.bucket_workspace_bytes(n, L, 1, records=True), dtype=torch.uint8, device=dev)
    st = {r: torch.empty(n, dtype=torch.uint8, device=dev) for r in routes}
    rep = {r: torch.empty((n, 2), dtype=torch.int64, device=dev).view(torch.uint8).view(n, 16) for r in routes}
    prec = P.bucket_put_records(keys[0], vals[0], 1, workspace=bws) if op != "cswap" else None
    grec = P.bucket_records(keys[0], 1, workspace=bws) if op == "cswap" else None
    mbits = [None] * nsets
    turn = {r: 0 for r in routes}
    calls = {r: 0 for r in routes}

    def fill():
        for r, tab in tabs.items():
            tab.clear()
            if present:
                tab.put_keys(keys[0], vals[0], status=st[r], workspace=ws)
            calls[r] = 0
    if op == "cswap":  # the digests a caller would have kept, in every set's order
        scratch = P.DeviceTable(cap, B, dev)
        for k in range(nsets):
            scratch.clear()
            mbits[k] = scratch.put_keys(keys[k], vals[k], status=st["keys"], mbits=True, workspace=ws)[1]
        del scratch
    fill()

    def prep(r):
        if op == "add" and not present:
            tabs[r].clear()

    def nxt(r):
        turn[r] = (turn[r] + 1) % nsets
        return turn[r]

    def pair(r):  # 0 -> 1, then 1 -> 0, ...: every request of a present key swaps
        calls[r] += 1
        return (0, 1) if calls[r] % 2 else (1, 0)

    def by_keys():
        k = nxt("keys")
        if op == "cswap":
            tabs["keys"].cswap_keys(keys[k], slot, *pair("keys"), out=rep["keys"], workspace=ws)
        else:
            getattr(tabs["keys"], op + "_keys")(keys[k], vals[k], status=st["keys"], workspace=ws)

    def by_records():
        k = nxt("records")
        if op == "cswap":
            P.bucket_records(keys[k], 1, out=grec, workspace=bws)
            tabs["records"].cswap(grec[0], slot, *pair("records"), out=rep["records"], workspace=ws)
        else:
            P.bucket_put_records(keys[k], vals[k], 1, out=prec, workspace=bws)
            getattr(tabs["records"], op + "_records")(prec[0], status=st["records"], workspace=ws)

    def by_mbits():
        k = nxt("mbits")
        tabs["mbits"].cswap(mbits[k], slot, *pair("mbits"), out=rep["mbits"], workspace=ws)

    fns = {"keys": by_keys, "records": by_records, "mbits": by_mbits}

    def equal():
        ok = True
        for k in range(nsets):
            for r in routes:
                turn[r] = k - 1
                prep(r)
                fns[r]()
            for r in routes[1:]:
                if op == "cswap":
                    ok &= bool(torch.equal(rep["keys"], rep[r]))
                else:
                    ok &= bool(torch.equal(st["keys"], st[r]))
                ok &= tabs["keys"].counts()[:3] == tabs[r].counts()[:3]
            if op == "cswap":
                ok &= int(rep["keys"][:, 0].sum()) == (n if present else 0)
            else:
                want = {("update", True): 0, ("update", False): 3, ("add", True): 4, ("add", False): 0}[op, present]
                ok &= bool(st["keys"].eq(want).all())
        progress(f"{op} equal: {ok}")
        return ok

    legs = {f"{op}_{r}": ((lambda r=r: prep(r)), fns[r]) for r in routes}
    return legs, equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keysizes", default="8,13,32")
    ap.add_argument("--elemsizes", default="8,40")
    ap.add_argument("--cases", default="empty,present")
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--n-m", type=int, default=16, help="keys per batch, in units of 2^20")
    ap.add_argument("--log2-capacity", type=int, default=25)
    ap.add_argument("--sets", type=int, default=3, help="input buffers a leg rotates over")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, cap = a.n_m * M, 1 << a.log2_capacity
    path = a.out or os.path.join(ROOT, "profiles", "table", f"keysrmwbench_{a.n_m}M.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for L in (int(x) for x in a.keysizes.split(",")):
            for E in (int(x) for x in a.elemsizes.split(",")):
                for case in a.cases.split(","):
                    B = P.put_record_bytes(L, E) - 24
                    ms, ok = {}, True
                    for op in a.ops.split(","):  # one operation's tables at a time
                        progress(f"keysize {L} elemsize {E} {case} {op}")
                        legs, equal = op_legs(op, L, E, n, cap, case, a.sets, dev)
                        ok &= equal()  # (also the warm-up of every leg)
                        torch.cuda.synchronize()
                        ms.update({k: [] for k in legs})
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
                        del legs, equal
                        torch.cuda.empty_cache()
                    med = {k: float(np.median(v)) for k, v in ms.items()}
                    row = {"keysize": L, "elemsize": E, "rowbytes": B, "case": case, "n": n, "capacity": cap,
                           "load": n / cap, "sets": a.sets, "equal": bool(ok),
                           "ms": {k: round(v, 4) for k, v in med.items()},
                           "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                           "max_ms": {k: round(max(v), 4) for k, v in ms.items()},
                           "Gkeys_s": {k: round(n / v / 1e6, 3) for k, v in med.items()},
                           "record_buffer_bytes": n * (24 + B), "cswap_record_bytes": n * P.bucket_record_bytes(L)}
                    for op in a.ops.split(","):
                        row[f"{op}_keys_vs_records"] = round(med[f"{op}_keys"] / med[f"{op}_records"], 3)
                    if "cswap" in a.ops.split(","):
                        row["cswap_keys_vs_mbits"] = round(med["cswap_keys"] / med["cswap_mbits"], 3)
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
