#!/usr/bin/env python3
"""The table's insert-if-absent against the calls a caller had without it and against a torch route: one
process, HIP events on the launch stream, the legs of a case interleaved round by round, medians; the result
of the add is compared with a torch route's before anything is timed.

  python tools/addbench.py [--rowbytes 16,40,64] [--cases new,present,hot] [--n-m 16] [--log2-capacity 25]
                           [--rounds 3] [--reps 3] [--out profiles/table/addbench_16M.jsonl]

The default is 16M records into capacity 2^25 (load 0.5), as tools/accbench.py.  Cases:
  new      16M distinct mbits into an emptied table (cleared outside the timed span): every record creates
  present  the same mbits, permuted, into the table that holds them all: nothing is created, no row written
  hot      90 % of the positions name one mbits, into an emptied table: the hot slot's first position is
           posted once per wave, one creator copies one row, the rest of the batch creates as in `new`

Legs (one JSON line per rowbytes and case; times are medians in ms):
  add            add_records with status
  add_rep        add_records with status and replies (three kernels)
  add_get        add_records, then get(head=8) of the same records: what add_rep saves is the probe of the get
  put            put_records of the same records into the same table: the parent's call (it overwrites)
  get            get(head=8) of the same records on the table as the case leaves it
  get_mask_put   get -> keep the records whose reply says absent -> put_records of those: the route without
                 add; the count of absent records is read on the host (put_records takes its m from there).
                 Correct for `new` and `present` only: in `hot` the duplicates of an absent mbits all pass the
                 mask and the LAST one wins
  t_sorted       torch: unique + first index (scatter amin) of the batch, searchsorted against the sorted
                 mbits of the table, cat + sort of the merged keys and a gather of the merged rows
equal: status 0 is given to exactly the first record of every mbits the table lacked (torch: unique +
scatter amin), 4 to all others; the replies are the rows of those first records (or the rows the table held)
and equal a get after the call.
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

SEED = 0xADD0ADD0ADD0ADD1
M = 1 << 20


def progress(what):
    print(f"  .. {what}", file=sys.stderr, flush=True)


def words(n, first, dev):
    return P.splitmix64_fill(SEED, first, n, device=dev)


def case_legs(B, n, cap, case, dev):
    S = 24 + B
    w = S // 8
    base = words(n * w, 0, dev).view(n, w)  # distinct mbits in word 2 (splitmix64 is a bijection of the counter)
    base_b = base.view(torch.uint8).view(n, S)
    tab = P.DeviceTable(cap, B, dev)
    ws = torch.empty(P.table_add_workspace_bytes(n), dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    rec = words(n * w, n * w, dev).view(n, w)
    rec[:, 2] = base[:, 2][torch.randperm(n, device=dev)]
    if case == "hot":
        rec[torch.rand(n, device=dev) < 0.9, 2] = base[7, 2]
    recb = rec.view(torch.uint8).view(n, S)
    q = rec[:, 2].contiguous()
    rep = torch.empty((n, 1 + B // 8), dtype=torch.int64, device=dev).view(torch.uint8).view(n, 8 + B)
    out8 = torch.empty_like(rep)
    present = case == "present"

    def prep():
        if not present:
            tab.clear()

    if present:
        tab.put_records(base_b, status=st, workspace=ws)
        assert int(st.count_nonzero()) == 0
        tk, order0 = torch.sort(base[:, 2])
        trows = base[:, 3:][order0].contiguous()
    else:
        tk = torch.empty(0, dtype=torch.int64, device=dev)
        trows = torch.empty((0, w - 3), dtype=torch.int64, device=dev)

    def t_sorted():
        uq, inv = torch.unique(q, return_inverse=True)
        first = torch.full((len(uq),), n, dtype=torch.int64, device=dev).scatter_reduce_(
            0, inv, torch.arange(n, device=dev), "amin")
        if len(tk):
            pos = torch.searchsorted(tk, uq).clamp_(max=len(tk) - 1)
            new = tk[pos] != uq
        else:
            new = torch.ones(len(uq), dtype=torch.bool, device=dev)
        keys = torch.cat([tk, uq[new]])
        rows = torch.cat([trows, rec[:, 3:][first[new]]])
        order = torch.argsort(keys)
        return keys[order], rows[order], first, inv, new

    def get_mask_put():
        tab.get(recb, head=8, out=out8)
        absent = torch.nonzero(out8[:, 0] == 0).ravel()  # (host-synchronous: the count)
        if len(absent):
            tab.put_records(rec[absent].view(torch.uint8).view(-1, S), workspace=ws)

    def add_get():
        tab.add_records(recb, status=st, workspace=ws)
        tab.get(recb, head=8, out=out8)

    def equal():
        prep()
        tab.add_records(recb, status=st, replies=rep, workspace=ws)
        tab.get(recb, head=8, out=out8)
        ok = bool(torch.equal(rep, out8))
        _, _, first, inv, new = t_sorted()
        want = torch.full((n,), 4, dtype=torch.uint8, device=dev)
        want[first[new]] = 0
        ok &= bool(torch.equal(st, want))
        rows = rep.view(torch.int64)[:, 1:]
        if present:
            ok &= bool(torch.equal(rows, trows[torch.searchsorted(tk, q)]))  # the rows the table held
        else:
            ok &= bool(torch.equal(rows, rec[:, 3:][first[inv]]))  # the first record's row, for every record
        ok &= tab.counts()[1] == 0
        progress(f"equal: {ok}")
        return ok

    legs = {
        "add": (prep, lambda: tab.add_records(recb, status=st, workspace=ws)),
        "add_rep": (prep, lambda: tab.add_records(recb, status=st, replies=rep, workspace=ws)),
        "add_get": (prep, add_get),
        "put": (prep, lambda: tab.put_records(recb, status=st, workspace=ws[:4 * n])),
        "get": (lambda: None, lambda: tab.get(recb, head=8, out=out8)),
        "get_mask_put": (prep, get_mask_put),
        "t_sorted": (lambda: None, t_sorted),
    }
    return legs, equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rowbytes", default="16,40,64")
    ap.add_argument("--cases", default="new,present,hot")
    ap.add_argument("--n-m", type=int, default=16, help="records per batch, in units of 2^20")
    ap.add_argument("--log2-capacity", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, cap = a.n_m * M, 1 << a.log2_capacity
    path = a.out or os.path.join(ROOT, "profiles", "table", f"addbench_{a.n_m}M.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for B in (int(x) for x in a.rowbytes.split(",")):
            for case in a.cases.split(","):
                progress(f"rowbytes {B} {case}")
                legs, equal = case_legs(B, n, cap, case, dev)
                ok = equal()
                torch.cuda.synchronize()
                ms = {k: [] for k in legs}
                for _ in range(a.rounds):
                    for k, (prep, fn) in legs.items():
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                              for _ in range(a.reps)]
                        for s, e in ev:
                            prep()
                            s.record()
                            fn()
                            e.record()
                        torch.cuda.synchronize()
                        ms[k].extend(s.elapsed_time(e) for s, e in ev)
                        progress(f"{k}: {ms[k][-1]:.3f} ms")
                med = {k: float(np.median(v)) for k, v in ms.items()}
                row = {"rowbytes": B, "case": case, "n": n, "capacity": cap, "load": n / cap, "equal": bool(ok),
                       "ms": {k: round(v, 4) for k, v in med.items()},
                       "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                       "Mrec_s": {k: round(n / v / 1e3, 1) for k, v in med.items()},
                       "add_vs_put": round(med["add"] / med["put"], 3),
                       "add_rep_vs_add_get": round(med["add_rep"] / med["add_get"], 3),
                       "get_mask_put_vs_add": round(med["get_mask_put"] / med["add"], 3),
                       "t_sorted_vs_add": round(med["t_sorted"] / med["add"], 3)}
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
                del legs, equal
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
