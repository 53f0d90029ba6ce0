#!/usr/bin/env python3
"""The table's update and compare-and-swap against what they should cost and against the torch route a
caller has without them: one process, HIP events on the launch stream, the legs of a shape interleaved
round by round, results compared for equality before anything is timed.

  python tools/rmwbench.py [--rowbytes 16,40,64] [--n-m 16] [--log2-capacity 25] [--rounds 3] [--reps 4]
                           [--out profiles/table/rmwbench_16M.jsonl]

The default is 16M requests into capacity 2^25 (load 0.5), as tools/tablebench.py.  Two request batches per
rowbytes: `distinct` (every mbits of the table once, permuted) and `hot` (90 % of the positions ask for one
mbits).  The swapped word is word 0 of the row; successive cswap calls swap A -> B and B -> A, so every call
finds its compare value in every requested entry and stores.

Legs (one JSON line per rowbytes and batch, times are medians in ms):
  update       update_records of the batch's records
  put_over     put_records of the same records (every mbits is present): what an update should cost
  cswap        cswap of the batch's mbits, replies at stride 16
  cswap_plain  the same through the tuning build's variant 340 (plain reply stores; the product's follow
               kTableReplyNt, non-temporal)
  get8         get, head 8, of the same mbits: a cswap should cost about this plus one atomic
  t_cswap      torch: stable sort of the mbits, first-of-run mask, searchsorted against the exported mbits,
               masked word gather and scatter
equal: update's table equals put's; cswap's replies and words equal the torch route's.
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

SEED = 0x7AB1E7AB1E7AB1E5
M = 1 << 20
A, Bv = 0x1111111111111111, 0x2222222222222222  # the flag pair


def words(n, first, dev):
    return P.splitmix64_fill(SEED, first, n, device=dev)


def shape_legs(B, n, cap, hot, dev):
    S = 24 + B
    w = S // 8
    base = words(n * w, 0, dev).view(n, w)
    base[:, 3] = A  # word 0 of every row
    tab = P.DeviceTable(cap, B, dev)
    ws = torch.empty(4 * n, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    tab.put_records(base.view(torch.uint8).view(n, S), status=st, workspace=ws)
    assert int(st.count_nonzero()) == 0
    # the batch: the table's mbits permuted, 90 % of them one mbits when hot; rows of its own
    perm = torch.randperm(n, device=dev)
    rec = words(n * w, n * w, dev).view(n, w)
    rec[:, 2] = base[:, 2][perm]
    rec[:, 3] = A
    if hot:
        rec[torch.rand(n, device=dev) < 0.9, 2] = base[7, 2]
    recb = rec.view(torch.uint8).view(n, S)
    q = rec[:, 2].contiguous()
    rep = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    out8 = torch.empty((n, 8 + B), dtype=torch.uint8, device=dev)
    # the torch route's table: sorted mbits and the word (exported once, outside the timing)
    tk, order0 = torch.sort(base[:, 2])
    tw = base[:, 3][order0].contiguous()
    turn = {"c": 0, "cp": 0, "t": 0}

    def pair(k):
        turn[k] += 1
        return (A, Bv) if turn[k] % 2 else (Bv, A)

    def t_cswap(tw, compare, desired):
        sq, order = torch.sort(q, stable=True)
        first_sorted = torch.ones(n, dtype=torch.bool, device=dev)
        first_sorted[1:] = sq[1:] != sq[:-1]
        first = torch.empty_like(first_sorted)
        first[order] = first_sorted
        pos = torch.searchsorted(tk, q).clamp_(max=n - 1)
        found = tk[pos] == q
        word = tw[pos]
        hit = word == compare
        old = torch.where(first | ~hit, word, torch.full_like(word, desired)) * found
        tw[pos[first & found & hit]] = desired
        return found, old

    def equal():
        ok = True
        # update == put over existing entries
        tab.update_records(recb, status=st, workspace=ws)
        ok &= int((st == 3).sum()) == 0
        st_u = st.clone()
        tab.get(base[:, 2].contiguous(), head=8, out=out8)
        after_u = out8.clone()
        tab.put_records(base.view(torch.uint8).view(n, S), status=st, workspace=ws)
        tab.put_records(recb, status=st, workspace=ws)
        tab.get(base[:, 2].contiguous(), head=8, out=out8)
        ok &= bool(torch.equal(st_u, st)) and bool(torch.equal(after_u, out8))
        # cswap == the torch route, twice (A -> B, then B -> A), product and plain stores
        tab.put_records(base.view(torch.uint8).view(n, S), status=st, workspace=ws)
        t = tw.clone()
        for i, (c, d) in enumerate(((A, Bv), (Bv, A), (A, Bv), (Bv, A))):
            found, old = t_cswap(t, c, d)
            rep.fill_(7)
            if i >= 2:
                with P.tuning(340):
                    tab.cswap(q, 0, c, d, out=rep, workspace=ws)
            else:
                tab.cswap(q, 0, c, d, out=rep, workspace=ws)
            r = rep.view(torch.int64)
            ok &= bool(torch.equal(r[:, 0], found.to(torch.int64))) and bool(torch.equal(r[:, 1], old))
            tab.get(tk, head=8, out=out8)
            ok &= bool(torch.equal(out8[:, 8:16].contiguous().view(torch.int64).view(-1), t))
        return ok

    tws = tw.clone()
    legs = {
        "update": lambda: tab.update_records(recb, status=st, workspace=ws),
        "put_over": lambda: tab.put_records(recb, status=st, workspace=ws),
        "cswap": lambda: tab.cswap(q, 0, *pair("c"), out=rep, workspace=ws),
        "cswap_plain": lambda: tab.cswap(q, 0, *pair("c"), out=rep, workspace=ws),
        "get8": lambda: tab.get(q, head=8, out=out8),
        "t_cswap": lambda: t_cswap(tws, *pair("t")),
    }
    return legs, {"cswap_plain": 340}, equal, tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rowbytes", default="16,40,64")
    ap.add_argument("--n-m", type=int, default=16, help="requests per batch, in units of 2^20")
    ap.add_argument("--log2-capacity", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4, help="even: the cswap legs alternate A -> B and B -> A")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, cap = a.n_m * M, 1 << a.log2_capacity
    path = a.out or os.path.join(ROOT, "profiles", "table", f"rmwbench_{a.n_m}M.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for B in (int(x) for x in a.rowbytes.split(",")):
            for hot in (False, True):
                legs, variant, equal, tab = shape_legs(B, n, cap, hot, dev)
                ok = equal()
                torch.cuda.synchronize()
                ms = {k: [] for k in legs}
                for _ in range(a.rounds):
                    for k, fn in legs.items():
                        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                              for _ in range(a.reps)]
                        with P.tuning(variant[k]) if k in variant else _null():
                            for s, e in ev:
                                s.record()
                                fn()
                                e.record()
                        torch.cuda.synchronize()
                        ms[k].extend(s.elapsed_time(e) for s, e in ev)
                med = {k: float(np.median(v)) for k, v in ms.items()}
                # per request: 8 B of mbits, a tag line, a 64-bit atomic on the winner word's
                # line, 4 B of slot written and read back, the row word's line read, 16 B of reply
                cswap_bytes = n * (8 + 64 + 64 + 4 + 4 + 64 + 16)
                row = {"rowbytes": B, "batch": "hot" if hot else "distinct", "n": n, "capacity": cap, "load": n / cap,
                       "equal": ok, "reply_stores": "non-temporal (cswap_plain: plain)",
                       "ms": {k: round(v, 4) for k, v in med.items()},
                       "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                       "Mreq_s": {k: round(n / v / 1e3, 1) for k, v in med.items()},
                       "cswap_lines_GBps": round(cswap_bytes / med["cswap"] / 1e6, 1),
                       "update_vs_put_over": round(med["update"] / med["put_over"], 3),
                       "cswap_vs_get8": round(med["cswap"] / med["get8"], 3),
                       "cswap_plain_vs_nt": round(med["cswap_plain"] / med["cswap"], 3),
                       "cswap_vs_torch": round(med["t_cswap"] / med["cswap"], 3)}
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
                del legs, equal, tab
                torch.cuda.empty_cache()


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *e):
        return False


if __name__ == "__main__":
    main()
