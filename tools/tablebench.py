#!/usr/bin/env python3
"""The device-resident table against the torch route a caller has without it:
one process, HIP events on the launch stream, the legs of a shape interleaved
round by round, inputs rotated over two sets, results compared for equality
before anything is timed.

  python tools/tablebench.py [--rowbytes 16,40,64] [--n-m 16] [--log2-capacity 25] [--rounds 3] [--reps 5]
                             [--out profiles/table/tablebench_16M.jsonl]

The default is 16M records into capacity 2^25 (load 0.5): the table is over
1 GiB and cannot sit in the 256 MiB Infinity Cache.  mbits are splitmix64
words (distinct), record stride 24 + rowbytes.

Legs per rowbytes (one JSON line each, times are medians in ms):
  put_empty      put_records into a table cleared just before (the clear is outside the timing)
  put_over       put_records over the same mbits with other rows
  put_over_plain the same through the tuning build's variant 341 (plain row stores; the product's are non-temporal)
  get_hit8 / get_miss8      get, head 8, dense mbits: every request found / none
  get_hit8_plain            get_hit8 through variant 340 (plain reply stores; the product's are non-temporal)
  get_hit1 / get_miss1      the same with head 1 (byte pieces)
  t_put          torch: stable sort of the mbits, last of each run, index_select of the rows
  t_get_hit / t_get_miss    torch: searchsorted in the sorted mbits, index_select, mask; reply = status column + rows
  RS             read_stream (non-temporal) over 1 GiB, for scale
equal: the table's replies to all 16M mbits equal the torch route's, for hits and misses, head 8 and head 1.
Rates are records per second; *_GBps counts the lines DESIGN.md §4.7 accounts for.
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


def words(n, first, dev):
    return P.splitmix64_fill(SEED, first, n, device=dev)


def shape_legs(B, n, cap, dev):
    S = 24 + B
    w = S // 8
    rec = [words(n * w, j * n * w, dev).view(n, w) for j in range(2)]
    rec[1][:, 2] = rec[0][:, 2]  # the same mbits, other rows
    recb = [r.view(torch.uint8).view(n, S) for r in rec]
    rows = [r[:, 24:].contiguous() for r in recb]  # what the torch route is handed
    mb = rec[0][:, 2].contiguous()
    perm = torch.randperm(n, device=dev)
    hit = [mb[perm], mb.flip(0).contiguous()]
    miss = [words(n, (5 + j) << 40, dev) for j in range(2)]
    tab = P.DeviceTable(cap, B, dev)
    ws = torch.empty(4 * n, dtype=torch.uint8, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    out8 = torch.empty((n, 8 + B), dtype=torch.uint8, device=dev)
    out1 = torch.empty((n, 1 + B), dtype=torch.uint8, device=dev)
    tout = torch.empty((n, 1 + B), dtype=torch.uint8, device=dev)
    stream_buf = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    fold = torch.zeros(1, dtype=torch.int64, device=dev)
    turn = {}

    def rot(leg):
        turn[leg] = turn.get(leg, -1) + 1
        return turn[leg] % 2

    def t_put(j):
        sm, order = torch.sort(mb, stable=True)
        last = torch.ones(n, dtype=torch.bool, device=dev)
        last[:-1] = sm[1:] != sm[:-1]
        return sm[last], rows[j].index_select(0, order[last])

    def t_get(tk, tr, q):
        pos = torch.searchsorted(tk, q).clamp_(max=tk.numel() - 1)
        found = tk[pos] == q
        tout[:, 0] = found
        tout[:, 1:] = tr.index_select(0, pos) * found[:, None]
        return tout

    tk, tr = t_put(0)
    state = {"tk": tk, "tr": tr}

    def leg_put(leg):
        tab.put_records(recb[rot(leg)], status=st, workspace=ws)

    legs = {
        "put_over": lambda: leg_put("put_over"),
        "put_over_plain": lambda: leg_put("put_over_plain"),
        "get_hit8": lambda: tab.get(hit[rot("h8")], head=8, out=out8),
        "get_hit8_plain": lambda: tab.get(hit[rot("h8p")], head=8, out=out8),
        "get_miss8": lambda: tab.get(miss[rot("m8")], head=8, out=out8),
        "get_hit1": lambda: tab.get(hit[rot("h1")], head=1, out=out1),
        "get_miss1": lambda: tab.get(miss[rot("m1")], head=1, out=out1),
        "t_put": lambda: t_put(rot("tp")),
        "t_get_hit": lambda: t_get(state["tk"], state["tr"], hit[rot("th")]),
        "t_get_miss": lambda: t_get(state["tk"], state["tr"], miss[rot("tm")]),
        "RS": lambda: P.read_stream(stream_buf, True, out=fold),
    }
    variant = {"put_over_plain": 341, "get_hit8_plain": 340}

    def equal():
        ok = True
        tab.put_records(recb[0], status=st, workspace=ws)
        ok &= int(st.count_nonzero()) == 0
        for j in (1, 0):  # over existing entries, twice; ends holding set 0 as the torch route does
            tab.put_records(recb[j], status=st, workspace=ws)
        ok &= tab.counts()[:3] == (n, 0, 3)
        for q in (hit[0], miss[0]):
            want = t_get(state["tk"], state["tr"], q)
            tab.get(q, head=1, out=out1)
            ok &= bool(torch.equal(out1, want))
            tab.get(q, head=8, out=out8)
            ok &= bool(torch.equal(out8[:, 8:], want[:, 1:])) and bool(torch.equal(out8[:, 0], want[:, 0]))
            ok &= int(out8[:, 1:8].count_nonzero()) == 0
            with P.tuning(340):
                out8.fill_(7)
                tab.get(q, head=8, out=out8)
            ok &= bool(torch.equal(out8[:, 8:], want[:, 1:])) and bool(torch.equal(out8[:, 0], want[:, 0]))
        with P.tuning(341):
            tab.put_records(recb[1], status=st, workspace=ws)
        tk1, tr1 = t_put(1)
        tab.get(tk1, head=8, out=out8)
        ok &= bool(torch.equal(out8[:, 8:], tr1))
        tab.put_records(recb[0], status=st, workspace=ws)
        return ok

    def put_empty(rounds, reps):
        ms = []
        for _ in range(rounds * reps):
            tab.clear()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            leg_put("put_empty")
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        probes = tab.counts()[3]
        tab.put_records(recb[0], status=st, workspace=ws)
        return ms, probes

    return legs, variant, equal, put_empty, tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rowbytes", default="16,40,64")
    ap.add_argument("--n-m", type=int, default=16, help="records per batch, in units of 2^20")
    ap.add_argument("--log2-capacity", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, cap = a.n_m * M, 1 << a.log2_capacity
    path = a.out or os.path.join(ROOT, "profiles", "table", f"tablebench_{a.n_m}M.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for B in (int(x) for x in a.rowbytes.split(",")):
            legs, variant, equal, put_empty, tab = shape_legs(B, n, cap, dev)
            ok = equal()
            torch.cuda.synchronize()
            ms = {k: [] for k in legs}
            ms["put_empty"], probes = put_empty(a.rounds, a.reps)
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
            # lines touched: put = record read + tag line + winner word line + row written;
            # get = mbits + tag line + row read + reply written
            put_bytes = n * ((24 + B) + 64 + 64 + B + 4 + 4 + 1)
            get_bytes = n * (8 + 64 + B + (8 + B))
            row = {"rowbytes": B, "n": n, "capacity": cap, "load": n / cap, "table_bytes": tab.nbytes, "equal": ok,
                   "probe_load": "relaxed agent-scope atomic load (sc1)", "reply_stores": "non-temporal",
                   "put_row_stores": "non-temporal",
                   "slots_per_record_empty": round(probes / n, 4),
                   "ms": {k: round(v, 4) for k, v in med.items()},
                   "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
                   "Mrec_s": {k: round(n / v / 1e3, 1) for k, v in med.items() if k != "RS"},
                   "put_over_GBps": round(put_bytes / med["put_over"] / 1e6, 1),
                   "get_hit8_GBps": round(get_bytes / med["get_hit8"] / 1e6, 1),
                   "put_over_vs_torch": round(med["t_put"] / med["put_over"], 3),
                   "get_hit8_vs_torch": round(med["t_get_hit"] / med["get_hit8"], 3),
                   "get_miss8_vs_torch": round(med["t_get_miss"] / med["get_miss8"], 3),
                   "read_stream_GBps": round((1 << 30) / med["RS"] / 1e6, 1)}
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            del legs, equal, put_empty, tab
            torch.cuda.empty_cache()


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *e):
        return False


if __name__ == "__main__":
    main()
