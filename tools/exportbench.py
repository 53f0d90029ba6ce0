#!/usr/bin/env python3
"""The table export against the torch route a caller has without it, and rehash against its two
halves: one process, HIP events on the launch stream, the legs of a shape interleaved round by round,
outputs rotated over two sets, results compared for equality before anything is timed.

  python tools/exportbench.py [--rowbytes 16,40,64] [--loads 0.1,0.5,0.9] [--log2-capacity 25]
                              [--rounds 3] [--reps 5] [--out profiles/table/export_bench.jsonl]

The default capacity is 2^25: the tags alone are 256 MiB and the table 1.0-2.5 GiB, so nothing sits in
the Infinity Cache.  mbits are splitmix64 words (distinct, none 0); a table is taken from load to load
by further puts.

Legs per (rowbytes, load), one JSON line each, times are medians in ms:
  dense / record          export of the whole table: three arrays / put records of stride 24 + rowbytes
  dense_nt / record_nt    the same through the tuning build's variant 342 (non-temporal output stores;
                          the product's are plain)
  dense_masks / record_masks   variant 343: the write pass reads the ballot masks the count pass saved
                          (1 bit per slot) instead of the tags again
  dense_tun               the product's kernels through the tuning build (variant 0): the base the two
                          variants are compared with
  count                   the count-only form (two launches)
  torch                   nonzero of the tags, index_select of the rows, a gather of the mbits
  RS                      read_stream (non-temporal) over 1 GiB, for scale
equal: the export's (mbits, rows, slots) equal the torch route's, for every variant and both forms.
GBps counts the algorithmic bytes of DESIGN.md §4.7: 8(C+1) tags in the count pass, 8(C+1) again in the
write pass ((C+1)/8 with masks), e*B row bytes read, e*(B+12) written (dense: e*(B+8) + 4e).

Then, per rowbytes: rehash 2^(log2-capacity - 1) -> 2^log2-capacity at load 0.5 of the small table
(host clock around the synchronous call) against export_records and put_records timed apart.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pdht_amd as P  # noqa: E402

SEED = 0x7AB1E7AB1E7AB1E5


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *e):
        return False


def words(n, first, dev):
    return P.splitmix64_fill(SEED, first, n, device=dev)


def put_more(tab, n, first, dev):
    """n further records of distinct mbits (splitmix words from `first` on)."""
    S = 24 + tab.rowbytes
    w = S // 8
    rec = words(n * w, first, dev).view(n, w).view(torch.uint8).view(n, S)
    st = tab.put_records(rec)
    assert int(st.count_nonzero()) == 0
    del rec, st


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return [s.elapsed_time(e) for s, e in ev]


def export_shape(tab, e, dev, rounds, reps):
    C, B = tab.capacity, tab.rowbytes
    S = 24 + B
    with P.tuning(343):
        need = P.table_export_workspace_bytes(C + 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    count = torch.empty(2, dtype=torch.int64, device=dev)
    mb = [torch.empty(e, dtype=torch.int64, device=dev) for _ in range(2)]
    rows = [torch.empty((e, B), dtype=torch.uint8, device=dev) for _ in range(2)]
    sl = [torch.empty(e, dtype=torch.int32, device=dev) for _ in range(2)]
    rec = [torch.empty((e, S), dtype=torch.uint8, device=dev) for _ in range(2)]
    tags = tab.storage[64:64 + 8 * (C + 1)].view(torch.int64)
    trows = tab.storage[64 + 16 * (C + 1):64 + (16 + B) * (C + 1)].view(C + 1, B)
    stream_buf = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    fold = torch.zeros(1, dtype=torch.int64, device=dev)
    turn = {}

    def rot(leg):
        turn[leg] = turn.get(leg, -1) + 1
        return turn[leg] % 2

    def dense(leg):
        j = rot(leg)
        tab.export(mb[j], rows[j], sl[j], count=count, workspace=ws)

    def record(leg):
        tab.export_records(rec[rot(leg)], count=count, workspace=ws)

    def t_route():
        idx = torch.nonzero(tags).squeeze(1)
        return tags[idx], trows.index_select(0, idx), idx

    legs = {
        "dense": lambda: dense("d"), "record": lambda: record("r"),
        "dense_tun": lambda: dense("dt"),
        "dense_nt": lambda: dense("dn"), "record_nt": lambda: record("rn"),
        "dense_masks": lambda: dense("dm"), "record_masks": lambda: record("rm"),
        "count": lambda: tab.export(None, count=count, workspace=ws),
        "torch": t_route,
        "RS": lambda: P.read_stream(stream_buf, True, out=fold),
    }
    variant = {"dense_tun": 0, "dense_nt": 342, "record_nt": 342, "dense_masks": 343, "record_masks": 343}

    ok = True
    tm, tr, ti = t_route()
    ok &= tm.numel() == e
    for v in (None, 0, 342, 343):
        with P.tuning(v) if v is not None else _null():
            for t in (mb[0], rows[0], sl[0], rec[0]):
                t.view(torch.uint8).fill_(0x5A)
            dense("eq")
            turn["eq"] = -1
            ok &= count.cpu().tolist() == [e, e]
            ok &= bool(torch.equal(mb[0], tm)) and bool(torch.equal(rows[0], tr)) and bool(torch.equal(sl[0], ti.int()))
            tab.export_records(rec[0], count=count, workspace=ws)
            ok &= bool(torch.equal(rec[0][:, 24:], tr)) and bool(torch.equal(rec[0][:, 16:24].contiguous().view(torch.int64)[:, 0], tm))
            ok &= bool(torch.equal(rec[0][:, 12:16].contiguous().view(torch.int32)[:, 0], ti.int()))
            ok &= int((rec[0][:, :12] != 0x5A).count_nonzero()) == 0
    del tm, tr, ti
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for k, fn in legs.items():  # warm-up of every shape
        with P.tuning(variant[k]) if k in variant else _null():
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in legs.items():
            with P.tuning(variant[k]) if k in variant else _null():
                ms[k].extend(timed(fn, reps))
    return ms, ok


def export_row(tab, e, ms, ok):
    C, B = tab.capacity, tab.rowbytes
    med = {k: float(np.median(v)) for k, v in ms.items()}
    tags2 = 16 * (C + 1)
    by = {"dense": tags2 + e * B + e * (B + 12), "record": tags2 + e * B + e * (B + 12),
          "masks": 8 * (C + 1) + (C + 1) // 8 + e * B + e * (B + 12), "count": 8 * (C + 1)}
    gbps = {k: round(by["masks" if k.endswith("masks") else "count" if k == "count" else "dense"] / med[k] / 1e6, 1)
            for k in med if k not in ("torch", "RS")}
    return {"bench": "export", "rowbytes": B, "capacity": C, "load": round(e / C, 3), "entries": e,
            "table_bytes": tab.nbytes, "equal": bool(ok), "output_stores": "plain", "liveness": "tags re-read",
            "bytes_per_slot": {k: round(v / (C + 1), 2) for k, v in by.items()},
            "ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
            "max_ms": {k: round(max(v), 4) for k, v in ms.items()}, "GBps": gbps,
            "dense_vs_torch": round(med["torch"] / med["dense"], 2),
            "record_vs_torch": round(med["torch"] / med["record"], 2),
            "nt_vs_plain_dense": round(med["dense_nt"] / med["dense_tun"], 3),
            "nt_vs_plain_record": round(med["record_nt"] / med["record"], 3),
            "masks_vs_tags_dense": round(med["dense_masks"] / med["dense_tun"], 3),
            "tuning_vs_product_dense": round(med["dense_tun"] / med["dense"], 3),
            "read_stream_GBps": round((1 << 30) / med["RS"] / 1e6, 1)}


def rehash_row(B, log2c, dev, reps):
    C0, C1 = 1 << (log2c - 1), 1 << log2c
    tab = P.DeviceTable(C0, B, dev)
    e = C0 // 2
    put_more(tab, e, 1 << 44, dev)
    S = 24 + B
    rec = torch.empty((C0 + 1, S), dtype=torch.uint8, device=dev)
    ws = torch.empty(P.table_export_workspace_bytes(C0 + 1), dtype=torch.uint8, device=dev)
    pws = torch.empty(4 * (C0 + 1), dtype=torch.uint8, device=dev)
    count = torch.empty(2, dtype=torch.int64, device=dev)
    big = P.DeviceTable(C1, B, dev)
    t_re, t_ex, t_put = [], [], []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new = tab.rehash(C1, storage=big.storage, chunk_bytes=1 << 40)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        ok = new.counts()[:3] == (e, 0, 1)
        ex = timed(lambda: tab.export_records(rec, count=count, workspace=ws), 1)[0]
        c = int(count.cpu()[1])
        big.clear()
        pt = timed(lambda: big.put_records(rec[:c], status=False, workspace=pws), 1)[0]
        if r:  # the first round warms up
            t_re.append(dt), t_ex.append(ex), t_put.append(pt)
    m = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    return {"bench": "rehash", "rowbytes": B, "from": C0, "to": C1, "entries": e, "equal": bool(ok), "chunks": 1,
            "ms": {"rehash_host_clock": m(t_re), "export_records": m(t_ex), "put_records": m(t_put)},
            "note": "rehash includes the new table's clear (a memset of its tags and winner words), the "
                    "allocation of its record buffer and one count read",
            "record_bytes": e * S, "Mentries_s": round(e / m(t_re) / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rowbytes", default="16,40,64")
    ap.add_argument("--loads", default="0.1,0.5,0.9")
    ap.add_argument("--log2-capacity", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C = 1 << a.log2_capacity
    path = a.out or os.path.join(ROOT, "profiles", "table", "export_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    loads = sorted(float(x) for x in a.loads.split(","))
    with open(path, "w") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for B in (int(x) for x in a.rowbytes.split(",")):
            tab, have = P.DeviceTable(C, B, dev), 0
            for load in loads:
                e = int(load * C)
                put_more(tab, e - have, (1 << 40) + have * ((24 + B) // 8), dev)
                have = e
                ms, ok = export_shape(tab, e, dev, a.rounds, a.reps)
                emit(export_row(tab, e, ms, ok))
                torch.cuda.empty_cache()
            del tab
            torch.cuda.empty_cache()
        for B in (int(x) for x in a.rowbytes.split(",")):
            emit(rehash_row(B, a.log2_capacity, dev, a.reps))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
