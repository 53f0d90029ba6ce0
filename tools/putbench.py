#!/usr/bin/env python3
"""Put records against what a caller had to do without them, and the row mover
against torch.index_select: one process, HIP events on the launch stream, the
legs of a shape interleaved round by round, inputs and outputs rotated over
sets larger than the 256 MiB Infinity Cache, outputs compared for equality
before anything is timed.

  python tools/putbench.py [--shapes 8:8:8,8:64:1024,...] [--n-m 16] [--rounds 3] [--reps 5]
  a shape is keysize:elemsize:nranks; the default is EXPERIMENTS.md §R8's list.

Legs per shape (one JSON line per shape, times are medians in ms):
  A     bucket_put_records (the product library; non-temporal mover stores)
  A330  the same through the tuning build's variant 330 (plain mover stores)
  R     bucket_records alone (A - R = what the values cost)
  B1-3  the route without put records, three times over: bucket_records, torch.index_select of the values
        by the records' index, strided copies of both into the wide records (pads pre-zeroed outside the
        timing); spread = max / min - 1 of the three medians
  G / G330 / T  gather_rows (product / plain stores) and torch.index_select on the same rows and index
  RS    read_stream (non-temporal) over 1 GiB, for scale
value_GBps = n x (E + round8(E)) bytes over A - R.  accept: A equals B byte for byte, and A's median is
no longer than B's by more than the spread.
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

SEED = 0x5EED5EED5EED5EED
M = 1 << 20
DEFAULT = ",".join(f"8:{E}:{nr}" for E in (8, 32, 64, 256) for nr in (8, 1024, 8192)) + ",32:64:1024"


def fill(nbytes, first, dev):
    return P.splitmix64_fill(SEED, first, nbytes // 8, device=dev).view(torch.uint8)


def shape_legs(L, E, nr, n, dev, sets):
    keys = [fill(n * L, j * n * L // 8, dev).view(n, L) for j in range(sets)]
    vals = [fill(n * E, (7 + j) * n * E // 8, dev).view(n, E) for j in range(sets)]
    with P.tuning(0):  # the tuning build reserves the two-pass intermediate at any nranks
        wsb = P.bucket_workspace_bytes(n, L, nr, records=True)
    ws = torch.empty(max(wsb, P.bucket_workspace_bytes(n, L, nr, records=True)), dtype=torch.uint8, device=dev)
    rb, rbk = P.put_record_bytes(L, E), P.bucket_record_bytes(L)
    outA = [P.bucket_put_records(keys[j], vals[j], nr, workspace=ws) for j in range(sets)]
    outR = [P.bucket_records(keys[j], nr, workspace=ws) for j in range(sets)]
    wide = [torch.zeros((n, rb), dtype=torch.uint8, device=dev) for _ in range(sets)]
    gat = torch.empty((n, E), dtype=torch.uint8, device=dev)
    sel = torch.empty((n, E), dtype=torch.uint8, device=dev)
    idx32 = [P.record_fields(outR[j][0], L)[3].contiguous() for j in range(sets)]
    idx64 = [(i.long() & 0xFFFFFFFF) for i in idx32]
    stream_buf = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    fold = torch.zeros(1, dtype=torch.int64, device=dev)
    turn = {}

    def rot(leg):
        turn[leg] = turn.get(leg, -1) + 1
        return turn[leg] % sets

    def leg_a(leg="A"):
        j = rot(leg)
        P.bucket_put_records(keys[j], vals[j], nr, out=outA[j], workspace=ws)

    def leg_r():
        j = rot("R")
        P.bucket_records(keys[j], nr, out=outR[j], workspace=ws)

    def leg_b(leg):
        j = rot(leg)
        rec, _ = P.bucket_records(keys[j], nr, out=outR[j], workspace=ws)
        ix = rec.view(-1).view(torch.int32).view(n, rbk // 4)[:, 3]
        torch.index_select(vals[j], 0, ix.long() & 0xFFFFFFFF, out=sel)
        wide[j][:, :rbk].copy_(rec)
        wide[j][:, rbk:rbk + E].copy_(sel)

    def leg_g(leg="G"):
        j = rot(leg)
        P.gather_rows(vals[j], idx32[j], out=gat, check=False)

    def leg_t():
        j = rot("T")
        torch.index_select(vals[j], 0, idx64[j], out=sel)

    legs = {"A": leg_a, "A330": (lambda: leg_a("A330")), "R": leg_r, "B1": (lambda: leg_b("B1")),
            "B2": (lambda: leg_b("B2")), "B3": (lambda: leg_b("B3")), "G": leg_g, "G330": (lambda: leg_g("G330")),
            "T": leg_t, "RS": (lambda: P.read_stream(stream_buf, True, out=fold))}

    def equal():
        """A == A330 == B byte for byte on every set, gather == index_select."""
        ok = True
        for j in range(sets):
            turn.update({"B1": j - 1, "A330": j - 1, "G": j - 1, "G330": j - 1, "T": j - 1})
            ref = outA[j][0].clone()
            leg_b("B1")
            ok &= bool(torch.equal(wide[j], ref)) and bool(torch.equal(outR[j][1], outA[j][1]))
            with P.tuning(330):
                leg_a("A330")
            ok &= bool(torch.equal(outA[j][0], ref))
            leg_t()
            leg_g("G")
            ok &= bool(torch.equal(gat, sel))
            gat.zero_()
            with P.tuning(330):
                leg_g("G330")
            ok &= bool(torch.equal(gat, sel))
        turn.clear()
        return ok

    return legs, equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--n-m", type=int, default=16, help="keys per batch, in units of 2^20")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.n_m * M
    for shape in a.shapes.split(","):
        L, E, nr = (int(x) for x in shape.split(":"))
        # sets: inputs and outputs of consecutive steps never share a line still in the Infinity Cache
        sets = max(2, -(-(1 << 30) // (n * (E + P.put_record_bytes(L, E)))))
        legs, equal = shape_legs(L, E, nr, n, dev, sets)
        ok = equal()
        legs["A"]()  # (the product's tag, read after a product call)
        tag = P.last_kernel()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(a.reps)]
                with P.tuning(330) if k.endswith("330") else _null():
                    for s, e in ev:
                        s.record()
                        f()
                        e.record()
                torch.cuda.synchronize()
                ms[k].extend(s.elapsed_time(e) for s, e in ev)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        bs = [med["B1"], med["B2"], med["B3"]]
        spread = max(bs) / min(bs) - 1
        b = float(np.median(bs))
        r8 = (E + 7) // 8 * 8
        vbytes = n * (E + r8)
        row = {"keysize": L, "elemsize": E, "nranks": nr, "n": n, "sets": sets, "kernel": tag, "equal": ok,
               "ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
               "B_ms": round(b, 4), "B_spread": round(spread, 4), "A_over_B": round(med["A"] / b, 4),
               "value_ms": round(med["A"] - med["R"], 4),
               "value_GBps": round(vbytes / max(med["A"] - med["R"], 1e-6) / 1e6, 1),
               "value_GBps_plain": round(vbytes / max(med["A330"] - med["R"], 1e-6) / 1e6, 1),
               "gather_GBps": round(2 * n * E / med["G"] / 1e6, 1),
               "gather_plain_GBps": round(2 * n * E / med["G330"] / 1e6, 1),
               "index_select_GBps": round(2 * n * E / med["T"] / 1e6, 1),
               "read_stream_GBps": round((1 << 30) / med["RS"] / 1e6, 1),
               "accept": bool(ok and med["A"] <= b * (1 + spread))}
        print(json.dumps(row), flush=True)
        del legs, equal
        torch.cuda.empty_cache()


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *e):
        return False


if __name__ == "__main__":
    main()
