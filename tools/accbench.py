#!/usr/bin/env python3
"""The table's accumulate against the calls a caller had without it and against a torch route: one process,
HIP events on the launch stream, the legs of a shape interleaved round by round, medians; the tables are
compared with the torch route for equality before anything is timed.

  python tools/accbench.py [--types i64,f64] [--elems 1,4] [--n-m 16] [--log2-capacity 25] [--rounds 3]
                           [--reps 4] [--out profiles/table/accbench_16M.jsonl]

The default is 16M records into capacity 2^25 (load 0.5), as tools/rmwbench.py.  A row is one 8-byte key
word and `elems` 8-byte counters behind it (rowbytes 16 or 40), the region at offset 8.  Two batches per
shape: `distinct` (every mbits of the table once, permuted) and `hot` (90 % of the positions name one mbits).
The addends are integers below 2^20 (as doubles for f64), so that every double sum is exact and the tables
can be compared bit for bit.

Legs (one JSON line per type, elems and batch; times are medians in ms):
  acc           acc_records, present-only (one kernel)
  acc_ins       acc_records(insert=True) on the same full table: every mbits is present, the claim probes only
  acc_ins_new   acc_records(insert=True) into an emptied table of the same capacity (cleared outside the
                timed span): every distinct mbits of the batch is created
  update        update_records of the same records: the parent's nearest call (it overwrites, it does not add)
  get_add_upd   get -> torch add on the replies -> update_records: the only route without acc; `distinct`
                only, the one batch for which it is correct
  t_index_add   torch: searchsorted against the sorted mbits + index_add_ into a dense [n, elems] array
  acc_nocomb    `hot` only: acc through the tuning build's variant 344 (every addend an atomic of its own)
equal: acc's and acc_ins_new's tables equal a torch route's on the same records (searchsorted / unique +
index_add_ of the same numbers as int64, exact, turned into the type's bits at the end), and acc_nocomb's too.
f64 on `hot` runs without t_index_add and acc_nocomb, the two legs that would post one double atomic per record
on one word (EXPERIMENTS.md R12 has the reason; variant 344 is built for the integer types only).
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

SEED = 0xACC0ACC0ACC0ACC1
M = 1 << 20
VO = 8


def progress(what):
    print(f"  .. {what}", file=sys.stderr, flush=True)


def words(n, first, dev):
    return P.splitmix64_fill(SEED, first, n, device=dev)


def shape_legs(kind, elems, n, cap, hot, dev):
    tdt = torch.int64 if kind == "i64" else torch.float64
    B = VO + 8 * elems
    S = 24 + B
    w = S // 8
    lo, hi = 3 + VO // 8, 3 + VO // 8 + elems  # the region's words inside a record

    def typed(x):  # integers below 2^20 in the type's bits
        v = (x & 0xFFFFF)
        return v if kind == "i64" else v.to(torch.float64).view(torch.int64)

    base = words(n * w, 0, dev).view(n, w)
    base_i = (base[:, lo:hi] & 0xFFFFF).contiguous()  # the same numbers as int64: the reference adds these
    base[:, lo:hi] = typed(base[:, lo:hi])
    tab = P.DeviceTable(cap, B, dev)
    ws = torch.empty(P.table_acc_workspace_bytes(n, True), dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    base_b = base.view(torch.uint8).view(n, S)
    tab.put_records(base_b, status=st, workspace=ws)
    assert int(st.count_nonzero()) == 0
    perm = torch.randperm(n, device=dev)
    rec = words(n * w, n * w, dev).view(n, w)
    rec[:, 2] = base[:, 2][perm]
    if hot:
        rec[torch.rand(n, device=dev) < 0.9, 2] = base[7, 2]
    add_i = (rec[:, lo:hi] & 0xFFFFF).contiguous()
    rec[:, lo:hi] = typed(rec[:, lo:hi])
    recb = rec.view(torch.uint8).view(n, S)
    q = rec[:, 2].contiguous()
    addv = rec[:, lo:hi].contiguous().view(tdt)
    # the torch route's table: sorted mbits and the dense counters (exported once, outside the timing)
    tk, order0 = torch.sort(base[:, 2])
    tw0 = base[:, lo:hi][order0].contiguous().view(tdt)
    tw0_i = base_i[order0].contiguous()
    # f64 on `hot`: the legs that post one double atomic per record on one word are left out (see the docstring)
    contended_ok = not (hot and kind == "f64")
    out8 = torch.empty((n, 8 + B), dtype=torch.uint8, device=dev)
    rec2 = rec.clone()
    rec2b = rec2.view(torch.uint8).view(n, S)
    empty = P.DeviceTable(cap, B, dev)

    def t_index_add(tw):
        pos = torch.searchsorted(tk, q)
        tw.index_add_(0, pos, addv)

    def bits(x_i):  # int64 sums (exact: every sum here stays below 2^53) as the table's bit patterns
        return x_i if kind == "i64" else x_i.to(torch.float64).view(torch.int64)

    def get_add_upd():
        tab.get(recb, head=8, out=out8)
        rec2[:, 3:] = out8.view(torch.int64)[:, 1:]
        region = rec2[:, lo:hi]
        region.copy_((region.contiguous().view(tdt) + addv).view(torch.int64))
        tab.update_records(rec2b, status=st, workspace=ws)

    def region_of(t, keys):
        t.get(keys, head=8, out=out8[:len(keys)])
        return out8[:len(keys)].view(torch.int64)[:, 1 + VO // 8:1 + VO // 8 + elems].contiguous()

    def equal():
        ok = True
        tw = tw0_i.clone()
        pos = torch.searchsorted(tk, q)
        for _ in range(2):  # present-only, twice
            tw.index_add_(0, pos, add_i)
            tab.acc_records(recb, tdt, VO, elems, status=st)
            ok &= int(st.count_nonzero()) == 0
            ok &= bool(torch.equal(region_of(tab, tk), bits(tw)))
        progress("equal: present-only")
        ok &= bool(torch.equal(out8.view(torch.int64)[:, 1], base[:, 3][order0]))  # the key word is untouched
        if hot and contended_ok:
            with P.tuning(344):
                tab.acc_records(recb, tdt, VO, elems, status=st)
            tw.index_add_(0, pos, add_i)
            ok &= bool(torch.equal(region_of(tab, tk), bits(tw)))
            progress("equal: no combining")
        # insert into the empty table: the distinct mbits, their sums, the first record's key word
        uq, inv = torch.unique(q, return_inverse=True)
        sums = torch.zeros((len(uq), elems), dtype=torch.int64, device=dev).index_add_(0, inv, add_i)
        first = torch.full((len(uq),), n, dtype=torch.int64, device=dev).scatter_reduce_(
            0, inv, torch.arange(n, device=dev), "amin")
        empty.clear()
        empty.acc_records(recb, tdt, VO, elems, insert=True, status=st, workspace=ws)
        ok &= int(st.count_nonzero()) == 0 and empty.counts()[0] == len(uq)
        ok &= bool(torch.equal(region_of(empty, uq), bits(sums)))
        ok &= bool(torch.equal(out8[:len(uq)].view(torch.int64)[:, 1], rec[:, 3][first]))
        progress("equal: insert")
        return ok

    tws = tw0.clone()
    nothing = lambda: None  # noqa: E731
    legs = {
        "acc": (nothing, lambda: tab.acc_records(recb, tdt, VO, elems, status=st)),
        "acc_ins": (nothing, lambda: tab.acc_records(recb, tdt, VO, elems, insert=True, status=st, workspace=ws)),
        "acc_ins_new": (empty.clear,
                        lambda: empty.acc_records(recb, tdt, VO, elems, insert=True, status=st, workspace=ws)),
        "update": (nothing, lambda: tab.update_records(recb, status=st, workspace=ws)),
    }
    if contended_ok:
        legs["t_index_add"] = (nothing, lambda: t_index_add(tws))
    if hot and contended_ok:
        legs["acc_nocomb"] = (nothing, lambda: tab.acc_records(recb, tdt, VO, elems, status=st))
    if not hot:
        legs["get_add_upd"] = (nothing, get_add_upd)
    return legs, {"acc_nocomb": 344}, equal, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="i64,f64")
    ap.add_argument("--elems", default="1,4")
    ap.add_argument("--batches", default="distinct,hot")
    ap.add_argument("--n-m", type=int, default=16, help="records per batch, in units of 2^20")
    ap.add_argument("--log2-capacity", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, cap = a.n_m * M, 1 << a.log2_capacity
    path = a.out or os.path.join(ROOT, "profiles", "table", f"accbench_{a.n_m}M.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for kind in a.types.split(","):
            for elems in (int(x) for x in a.elems.split(",")):
                for hot in (b == "hot" for b in a.batches.split(",")):
                    progress(f"{kind} elems {elems} {'hot' if hot else 'distinct'}")
                    legs, variant, equal, B = shape_legs(kind, elems, n, cap, hot, dev)
                    ok = equal()
                    torch.cuda.synchronize()
                    ms = {k: [] for k in legs}
                    for _ in range(a.rounds):
                        for k, (prep, fn) in legs.items():
                            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                                  for _ in range(a.reps)]
                            with P.tuning(variant[k]) if k in variant else _null():
                                for s, e in ev:
                                    prep()
                                    s.record()
                                    fn()
                                    e.record()
                            torch.cuda.synchronize()
                            ms[k].extend(s.elapsed_time(e) for s, e in ev)
                            progress(f"{k}: {ms[k][-1]:.3f} ms")
                    med = {k: float(np.median(v)) for k, v in ms.items()}
                    row = {"type": kind, "elems": elems, "rowbytes": B, "batch": "hot" if hot else "distinct", "n": n,
                           "capacity": cap, "load": n / cap, "equal": bool(ok),
                           "ms": {k: round(v, 4) for k, v in med.items()},
                           "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                           "Mrec_s": {k: round(n / v / 1e3, 1) for k, v in med.items()},
                           "added_GBps": round(n * elems * 8 / med["acc"] / 1e6, 1),
                           "acc_vs_update": round(med["acc"] / med["update"], 3),
                           "acc_ins_vs_acc": round(med["acc_ins"] / med["acc"], 3)}
                    for k, name in (("t_index_add", "torch_vs_acc"), ("acc_nocomb", "nocomb_vs_acc"),
                                    ("get_add_upd", "get_add_upd_vs_acc")):
                        if k in med:
                            row[name] = round(med[k] / med["acc"], 3)
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                    del legs, equal
                    torch.cuda.empty_cache()


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *e):
        return False


if __name__ == "__main__":
    main()
