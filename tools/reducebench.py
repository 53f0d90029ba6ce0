#!/usr/bin/env python3
"""The table's reduce (min, max, or) against the sum of the same records, against the calls a caller had
without it and against a torch route: one process, HIP events on the launch stream, the legs of a shape
interleaved round by round, medians; the tables are compared with a torch computation for equality before
anything is timed.  In the manner of tools/accbench.py.

  python tools/reducebench.py [--cases i64:min,i64:max,f64:min,f64:max,i64:or] [--elems 1,4] [--n-m 16]
                              [--log2-capacity 25] [--rounds 3] [--reps 4]
                              [--out profiles/table/reducebench_16M.jsonl]

The default is 16M records into capacity 2^25 (load 0.5).  A row is one 8-byte key word and `elems` 8-byte
words behind it (rowbytes 16 or 40), the region at offset 8.  Two batches per shape: `distinct` (every mbits
of the table once, permuted) and `hot` (90 % of the positions name one mbits).  Operands: random int64 of
both signs, as finite non-zero doubles for f64; 4 random bits per word for `or`.

Legs (one JSON line per type, op, elems and batch; times are medians in ms):
  red           reduce_records(op), present-only (one kernel)
  add           reduce_records("add") of the same records: the accumulate's kernel, the natural yardstick
                (the region's bits are summed as the type's numbers; for f64 on `hot` it is left out: what a
                hot double sum costs is tools/accbench.py's to say, with addends chosen for it)
  red_ins       reduce_records(op, insert=True) on the same full table: the claim probes only
  red_rep       reduce_records(op, replies=...): the slot store and the reply kernel on top
  red_get       reduce_records(op) followed by get of the same records: what the replies save
  get_op_upd    get -> torch min / max / or on the replies -> update_records: the only route without the
                call; `distinct` only, the one batch for which it is correct
  t_scatter     torch: searchsorted against the sorted mbits + scatter_reduce_ (amin / amax) into a dense
                [n, elems] array; `distinct` only, min and max only (torch has no scatter `or`)
NOT run, on purpose: any leg without the in-wave combining on doubles; a hot batch on a region of more than
32 elements; a torch scatter on the hot batch (one atomic per record on one word; for doubles that shape is
unmeasured on this part, EXPERIMENTS.md R12).
equal: red's table equals a torch computation on the same records (element-wise where every mbits comes once,
a tree fold over the hot mbits' operands), and the replies of red_rep equal a get after it.
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

SEED = 0x7ED0CE7ED0CE7ED1
M = 1 << 20
VO = 8


def progress(what):
    print(f"  .. {what}", file=sys.stderr, flush=True)


def words(n, first, dev):
    return P.splitmix64_fill(SEED, first, n, device=dev)


def fold(v, fn):
    """fn over the rows of v [k, elems], as a tree (no atomics)."""
    while len(v) > 1:
        h = len(v) // 2
        head = fn(v[:h], v[h:2 * h])
        v = torch.cat([head, v[2 * h:]]) if len(v) % 2 else head
    return v[0]


def shape_legs(kind, op, elems, n, cap, hot, dev):
    tdt = torch.int64 if kind == "i64" else torch.float64
    B = VO + 8 * elems
    S = 24 + B
    w = S // 8
    lo, hi = 3 + VO // 8, 3 + VO // 8 + elems  # the region's words inside a record
    fn = {"min": torch.minimum, "max": torch.maximum, "or": torch.bitwise_or}[op]

    def typed(x):  # random words -> the operands' bits
        if op == "or":
            return x & (x >> 17) & (x >> 31) & (x >> 5)  # a few bits each
        if kind == "i64":
            return x
        return ((x >> 11) | 1).to(torch.float64).mul_(torch.where(x & 1 == 1, 1.0, -1.0)).view(torch.int64)

    base = words(n * w, 0, dev).view(n, w)
    base[:, lo:hi] = typed(base[:, lo:hi])
    tab = P.DeviceTable(cap, B, dev)
    ws = torch.empty(P.table_reduce_workspace_bytes(n, True, True), dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    tab.put_records(base.view(torch.uint8).view(n, S), status=st, workspace=ws)
    assert int(st.count_nonzero()) == 0
    perm = torch.randperm(n, device=dev)
    rec = words(n * w, n * w, dev).view(n, w)
    rec[:, 2] = base[:, 2][perm]
    if hot:
        rec[torch.rand(n, device=dev) < 0.9, 2] = base[7, 2]
    rec[:, lo:hi] = typed(rec[:, lo:hi])
    recb = rec.view(torch.uint8).view(n, S)
    q = rec[:, 2].contiguous()
    opv = rec[:, lo:hi].contiguous().view(tdt)
    tk, order0 = torch.sort(base[:, 2])
    tw0 = base[:, lo:hi][order0].contiguous().view(tdt)
    out8 = torch.empty((n, 8 + B), dtype=torch.uint8, device=dev)
    rep8 = torch.empty((n, 8 + B), dtype=torch.uint8, device=dev)
    rec2 = rec.clone()
    rec2b = rec2.view(torch.uint8).view(n, S)

    def t_scatter(tw):
        pos = torch.searchsorted(tk, q)
        tw.scatter_reduce_(0, pos.unsqueeze(1).expand(-1, elems), opv, "amin" if op == "min" else "amax")

    def get_op_upd():
        tab.get(recb, head=8, out=out8)
        rec2[:, 3:] = out8.view(torch.int64)[:, 1:]
        region = rec2[:, lo:hi]
        region.copy_(fn(region.contiguous().view(tdt), opv).view(torch.int64))
        tab.update_records(rec2b, status=st, workspace=ws)

    def red_get():
        tab.reduce_records(recb, tdt, op, VO, elems, status=st)
        tab.get(recb, head=8, out=out8)

    def equal():
        tw = tw0.clone()
        pos = torch.searchsorted(tk, q)
        mine = q == base[7, 2] if hot else torch.zeros(n, dtype=torch.bool, device=dev)
        once = ~mine  # (every other mbits comes once: the permutation)
        tw[pos[once]] = fn(tw[pos[once]], opv[once])
        if hot:
            h = int(torch.searchsorted(tk, base[7:8, 2]))
            tw[h] = fn(tw[h], fold(opv[mine], fn))
        tab.reduce_records(recb, tdt, op, VO, elems, status=st, replies=rep8, workspace=ws)
        ok = int(st.count_nonzero()) == 0
        tab.get(tk, head=8, out=out8)
        ok &= bool(torch.equal(out8.view(torch.int64)[:, 2:2 + elems], tw.view(torch.int64)))
        ok &= bool(torch.equal(out8.view(torch.int64)[:, 1], base[:, 3][order0]))  # the key word is untouched
        tab.get(recb, head=8, out=out8)
        ok &= bool(torch.equal(out8, rep8))  # reply p = a get after the call
        progress(f"equal: {ok}")
        return ok

    tws = tw0.clone()
    legs = {
        "red": lambda: tab.reduce_records(recb, tdt, op, VO, elems, status=st),
        "red_ins": lambda: tab.reduce_records(recb, tdt, op, VO, elems, insert=True, status=st, workspace=ws),
        "red_rep": lambda: tab.reduce_records(recb, tdt, op, VO, elems, status=st, replies=rep8, workspace=ws),
        "red_get": red_get,
    }
    if not (hot and kind == "f64"):
        legs["add"] = lambda: tab.reduce_records(recb, tdt, "add", VO, elems, status=st)
    if not hot:
        legs["get_op_upd"] = get_op_upd
        if op != "or":
            legs["t_scatter"] = lambda: t_scatter(tws)
    return legs, equal, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="i64:min,i64:max,f64:min,f64:max,i64:or")
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
    path = a.out or os.path.join(ROOT, "profiles", "table", f"reducebench_{a.n_m}M.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for case in a.cases.split(","):
            kind, op = case.split(":")
            assert kind in ("i64", "f64") and op in ("min", "max", "or") and not (kind == "f64" and op == "or")
            for elems in (int(x) for x in a.elems.split(",")):
                assert elems <= 32, "hot batches are measured for regions the waves combine (at most 32 elements)"
                for hot in (b == "hot" for b in a.batches.split(",")):
                    progress(f"{kind} {op} elems {elems} {'hot' if hot else 'distinct'}")
                    legs, equal, B = shape_legs(kind, op, elems, n, cap, hot, dev)
                    ok = equal()
                    torch.cuda.synchronize()
                    ms = {k: [] for k in legs}
                    for _ in range(a.rounds):
                        for k, fn in legs.items():
                            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                                  for _ in range(a.reps)]
                            for s, e in ev:
                                s.record()
                                fn()
                                e.record()
                            torch.cuda.synchronize()
                            ms[k].extend(s.elapsed_time(e) for s, e in ev)
                            progress(f"{k}: {ms[k][-1]:.3f} ms")
                    med = {k: float(np.median(v)) for k, v in ms.items()}
                    row = {"type": kind, "op": op, "elems": elems, "rowbytes": B, "batch": "hot" if hot else "distinct",
                           "n": n, "capacity": cap, "load": n / cap, "equal": bool(ok),
                           "ms": {k: round(v, 4) for k, v in med.items()},
                           "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                           "Mrec_s": {k: round(n / v / 1e3, 1) for k, v in med.items()},
                           "rep_vs_red_get": round(med["red_rep"] / med["red_get"], 3),
                           "red_ins_vs_red": round(med["red_ins"] / med["red"], 3)}
                    for k, name in (("add", "red_vs_add"), ("get_op_upd", "red_vs_get_op_upd"),
                                    ("t_scatter", "red_vs_torch")):
                        if k in med:
                            row[name] = round(med["red"] / med[k], 3)
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                    del legs, equal
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
