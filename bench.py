#!/usr/bin/env python3
"""Benchmark: device-resident batch CityHash64 on 64-byte keys (BASELINE.json).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
                  [--config cfg1|cfg2|cfg3|cfg4|cfg5|place|bucket|exchange|records|xrecords|long]

A plain run does what the headline figure needs and nothing else: it sets up
the keys, warms up, times the K steps, writes the last step's outputs when
--dump-outputs is given and prints the line (contract fields, ms_per_step and
the roofline figures that follow from the timed steps themselves).  `--full`
adds every other leg described below: the configs[4] block, the calibrated
streams of the roofline block, cpu_baseline, host_resident, per_rank and
parity.

One step = one pass of the hot path (one kernel launch) over this GPU's batch
of synthetic keys already resident in HBM.  Default workload = BASELINE
configs[1] ("cfg2": 16M x 64 B keys per GPU, CityHash64).  For N > 1 (one rank
per GPU: `python bench.py --gpus N` starts the N ranks itself through
torch.distributed.run; under an external launcher WORLD_SIZE must equal N)
rank r hashes its own contiguous
slice [r*n, (r+1)*n) of the same key stream (pdht_amd.dist.weak_shard): no
collective on the data path (weak scaling); the only collectives are the
timing barrier, the max of elapsed times and the parity reductions.
"cfg5" = 128M keys per GPU, i.e. BASELINE configs[4] (1B keys) at N = 8.

The default config's --full run also times BASELINE configs[4] at its own N: the 1B x 64 B
stream split contiguously over the N ranks (1B/N keys per GPU, strong
scaling; "baseline_config4" block, parity from the committed 16M-key chunk
folds).  `--dist-backend gloo` rehearses the N-rank path on fewer GPUs (ranks
share devices; RCCL refuses two ranks on one GPU).

Rank 0 prints one JSON line.  Besides the contract fields it carries (all but
the first part of roofline only with --full)
  roofline      -- achieved algorithmic HBM GB/s of the hash kernel (72 B/key:
                   64 B key read + 8 B digest write) over its average step
                   time: one pair of HIP events on the launch stream around
                   the K timed steps (launches queued back to back),
                   plus HBM traffic per launch from the committed rocprofv3
                   PMC pass (profiles/traffic_<cfg>.json), a calibrated
                   read-stream rate on the same buffer and (64-B configs) the
                   kernel's own data movement with the hash replaced by an
                   XOR fold (calibrated_key_stream_GBps);
  cpu_baseline  -- the reference city.c (oracle/_ref, or the oracle port when
                   _ref is absent) timed on this host's cores over a bounded
                   sample of the same keys, as BASELINE.md §3 specifies: cfg1
                   one thread through per-key pdht_hash semantics (digest + both
                   reductions of hash.c:27/:29), every other config all the
                   cores this job may use (affinity capped by the cgroup CPU
                   quota), CLOCK_MONOTONIC_RAW, best of 5 (rank 0, N = 1 only);
  host_resident -- the same hash with keys/digests in pinned host memory
                   (zero-copy over PCIe); at N > 1 every rank measures its own
                   GPU at the same time (one PCIe link each) -> per-rank rates
                   and the aggregate;
  per_rank      -- (N > 1) each rank's device, kernel time, Gkeys/s and
                   roofline fraction, plus the RCCL world;
  parity        -- this run's digests of the whole shard checked against the
                   reference golden folds (tests/golden/config_folds.json);
                   no oracle code runs outside the cpu_baseline leg.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

M = 1 << 20
SEED_KEYS = 0x5EED5EED5EED5EED
SEED_LENS = 0x1E575EED1E575EED
PEAK_HBM_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
METRIC = "Gkeys/s and achieved HBM GB/s, device-resident batch CityHash64 on 64B keys"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="GPUs (= ranks) of this node; without WORLD_SIZE in the environment and N > 1 "
                         "bench.py starts the N ranks itself (torch.distributed.run, 127.0.0.1)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="cfg2",
                    choices=["cfg1", "cfg2", "cfg2r", "cfg3", "cfg4", "cfg5", "config4", "place", "bucket", "bucket8k",
                             "exchange", "records", "xrecords", "long"],
                    help="workload of the line (default cfg2 = BASELINE configs[1]); config4 = BASELINE configs[4] "
                         "alone as the line's workload: the 1B x 64 B stream split over the N ranks (strong "
                         "scaling), without the cfg2 leg -- what a profile of configs[4] alone runs")
    ap.add_argument("--keys-per-gpu", type=int, default=0, help="override the per-GPU batch")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=0.5,
                    help="wall budget of one CPU-baseline pass (best of 5 passes)")
    ap.add_argument("--dist-backend", default=None, choices=["nccl", "gloo"],
                    help="collective backend: nccl (= RCCL, one GPU per rank; the default at N > 1) or gloo (a "
                         "rehearsal: ranks share the visible GPUs round-robin, collectives on CPU tensors).  "
                         "Given at N = 1, the one rank still joins a process group of that backend, so the "
                         "collectives (and the exchange of the exchange/xrecords configs) run through it")
    ap.add_argument("--no-config4", action="store_true",
                    help="skip the BASELINE configs[4] block (1B x 64 B keys split over the N ranks)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg of the line: the parity check against "
                         "the reference folds, the calibrated read/key streams of the roofline block, the "
                         "host-resident rate, the CPU baseline, the per-rank block, cfg1's wrapper path and (default "
                         "config) the BASELINE configs[4] block.  Without it the run sets up, warms up, times the "
                         "steps and prints the line with the headline fields only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed (the arrays its caller "
                         "receives) as DIR/<name>.npy in float64/float32, a fixed seeded sample of the rows of a "
                         "large array (at most 64 MB in all); <name>.rank<r>.npy for ranks r > 0")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch check only: every rank joins a gloo group, touches no GPU and rank 0 "
                         "prints one JSON line with the world (tests/test_bench_launch.py)")
    return ap.parse_args()


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n: int) -> int:
    """`bench.py --gpus N` started as one process: start the N ranks (one per
    GPU) with torch.distributed.run and relay rank 0's JSON line.  This parent
    never touches a GPU (no torch import at all): it only forwards the ranks'
    other output to stderr and exits with the launcher's return code, which is
    non-zero as soon as any rank failed.  The ranks rendezvous on 127.0.0.1."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts
    env.setdefault("OMP_NUM_THREADS", "1")
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = []
    for line in p.stdout:
        s = line.strip()
        if s.startswith("{"):
            try:
                if isinstance(json.loads(s), dict):
                    lines.append(s)
                    continue
            except ValueError:
                pass
        sys.stderr.write(line)
    rc = p.wait()
    for s in lines:
        print(s, flush=True)
    if rc == 0 and len(lines) != 1:
        sys.stderr.write(f"bench.py: expected one JSON line from rank 0, got {len(lines)}\n")
        return 1
    return rc


def dry_run(a) -> None:
    """Launch check without a GPU: a gloo group of all ranks, every rank's
    (rank, local rank, pid) gathered, one JSON line from rank 0."""
    import torch.distributed as dist
    from pdht_amd import dist as D
    rank, local, world = D.env_rank_world()
    if world > 1:
        dist.init_process_group("gloo")
    mine = {"rank": rank, "local_rank": local, "pid": os.getpid()}
    allr = [mine]
    if world > 1:
        allr = [None] * world
        dist.all_gather_object(allr, mine)
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "world_size": world, "ranks": allr,
                          "gpus_arg": a.gpus, "backend": dist.get_backend() if world > 1 else None,
                          "plan": plan(a, world)}),
              flush=True)
    if world > 1:
        dist.destroy_process_group()


CONFIG4_KEYS = 1 << 30  # BASELINE configs[4]: 1B x 64 B keys over the node's GPUs


def plan(a, world: int) -> dict:
    """What this run measures, decided before any GPU work (printed by
    --dry-run, so the CPU tests can check it): the per-GPU workload of
    `value` and, for a --full run of the default config, the BASELINE
    configs[4] block -- the 1B x 64 B stream split over the N ranks (strong
    scaling), timed beside the cfg2 weak-scaling value at every N."""
    p = {"config": a.config, "value_scaling": "strong" if a.config == "config4" else "weak",
         "world_size": world, "backend": a.dist_backend}
    if a.config == "cfg2" and a.full and not a.no_config4 and not a.keys_per_gpu:
        p["config4"] = {"keys_total": CONFIG4_KEYS, "key_bytes": 64, "split": "strong (contiguous, 1B/N per rank)",
                        "keys_per_rank": [CONFIG4_KEYS * (r + 1) // world - CONFIG4_KEYS * r // world
                                          for r in range(world)]}
    return p


# Inputs that fit the 256 MiB Infinity Cache would be re-read from it by the
# next step (the same keys every step), not from HBM: such configs rotate
# over copies of their keys (and bucketing over output sets too, whose
# write-back stores could otherwise be overwritten in the cache before they
# reach HBM), so that >= 512 MiB pass between two uses of one buffer.
ROT_BYTES = 512 << 20


def rot_copies(torch, t, max_copies: int = 8) -> list:
    """t and enough identical copies that ROT_BYTES pass between two reads of
    one of them (a buffer of >= ROT_BYTES is used alone)."""
    nb = t.numel() * t.element_size()
    k = min(max_copies, max(1, -(-ROT_BYTES // max(nb, 1))))
    return [t] + [t.clone() for _ in range(k - 1)]


def flush_infinity_cache(torch, dev):
    """Write 512 MiB of scratch: the stores allocate in the 256 MiB Infinity
    Cache and evict whatever the set-up left there (the freshly generated
    keys); kernels whose loads are non-temporal never bring their inputs back,
    so every timed step reads them from HBM."""
    scratch = torch.empty(ROT_BYTES, dtype=torch.uint8, device=dev)
    scratch.fill_(0x5A)
    torch.cuda.synchronize()
    del scratch


DUMP_BYTES = 48 << 20  # all files of one --dump-outputs together (the limit is 64 MB), split evenly over the arrays
DUMP_SEED = 0x0D0C5EED


def dump_outputs(torch, path: str, arrays: dict, rank: int = 0) -> dict:
    """Write the tensors of `arrays` (name -> tensor or None) as
    <path>/<name>.npy (<name>.rank<r>.npy for rank r > 0) so that two builds
    can be compared value for value.  Every value is stored exactly: a 64-bit
    integer column becomes two float64 columns (its high and low 32 bits, both
    as unsigned numbers), narrower integers one float64 column, bytes float32.
    An array whose rows would exceed its share of DUMP_BYTES is cut to a
    fixed sample of its rows: the first and the last row and rows drawn by a
    generator seeded with DUMP_SEED (the same rows in every run of the same
    shape, in increasing order)."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: t for k, t in arrays.items() if torch.is_tensor(t)}
    share = DUMP_BYTES // max(1, len(arrays))
    done, total = {}, 0
    for name, t in arrays.items():
        t = t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(-1, 1)
        rows, cols = t.shape
        wide = t.dtype == torch.int64
        cell = 4 if t.dtype == torch.uint8 else (16 if wide else 8)
        keep = max(2, share // (cell * max(cols, 1)))
        if rows > keep:
            pick = np.random.default_rng(DUMP_SEED).integers(0, rows, size=keep - 2)
            idx = np.unique(np.concatenate(([0, rows - 1], pick)))
            t = t[torch.from_numpy(idx).to(t.device)]
        h = t.cpu().numpy()
        if wide:
            u = h.view(np.uint64)
            h = np.stack([(u >> np.uint64(32)).astype(np.float64),
                          (u & np.uint64(0xFFFFFFFF)).astype(np.float64)], axis=-1).reshape(h.shape[0], 2 * cols)
        elif h.dtype == np.uint8:
            h = h.astype(np.float32)
        else:
            h = h.astype(np.float64)
        f = os.path.join(path, f"{name}.npy" if rank == 0 else f"{name}.rank{rank}.npy")
        np.save(f, h)
        total += h.nbytes
        done[name] = {"file": os.path.basename(f), "rows": int(h.shape[0]), "of": int(rows), "dtype": str(h.dtype)}
    assert total <= 64 * 10 ** 6, total
    return {"dir": path, "bytes": total, "arrays": done}


def golden_folds():
    p = os.path.join(ROOT, "tests", "golden", "config_folds.json")
    if not os.path.exists(p):
        return None
    with open(p) as f:
        return json.load(f)["configs"]


def main():
    a = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is not None:
        if a.gpus is not None and int(env_world) != a.gpus:
            sys.stderr.write(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={env_world}: refusing to run a "
                             f"different world than asked for\n")
            sys.exit(2)
    elif a.gpus is not None and a.gpus > 1:
        sys.exit(launch_ranks(a.gpus))  # before anything touches a GPU
    if a.config == "config4" and a.keys_per_gpu:
        sys.stderr.write("bench.py: --config config4 is BASELINE configs[4] (1B keys split over the ranks); "
                         "--keys-per-gpu does not apply to it\n")
        sys.exit(2)
    if a.dry_run:
        dry_run(a)
        return
    import torch
    import torch.distributed as dist

    from pdht_amd import dist as D

    rank, local, world = D.env_rank_world()
    backend = a.dist_backend or ("nccl" if world > 1 else None)
    if world == 1 and backend is not None:
        # one rank in a group of one: every collective of the N-rank path
        # (barrier, max of times, parity reductions, per-rank gathers and the
        # exchange's all-to-all(v)) runs through the backend -- on one GPU box
        # the only way to execute the RCCL path on device tensors
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if backend == "gloo":
        # rehearsal of the N-rank path on fewer GPUs (e.g. 2 ranks on the one
        # GPU of a gpurun box, where RCCL refuses two ranks per device): ranks
        # share devices round-robin, the collectives run on CPU tensors
        torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
        dist.init_process_group("gloo")
    elif backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        torch.cuda.set_device(0)
    a.dist_backend = backend
    dev = torch.device("cuda", torch.cuda.current_device())
    cdev = dev if backend == "nccl" else None  # where the collectives' tensors live

    if not os.path.exists(os.path.join(ROOT, "pdht_amd", "lib", "libpdht_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    import pdht_amd as P

    cfg = a.config
    # ---------------------------------------------------------- workload ---
    keys = out = data = offs = None
    bucketed = None
    rotation = None  # set by configs whose inputs fit the Infinity Cache (rot_copies)
    if cfg in ("records", "xrecords"):
        # f4 in the MPI wire format: one message_t record (header + key) per
        # key at its bucketed position; "xrecords" buckets by the world size
        # and ships every bucket to its owner in ONE all-to-all(v) (RCCL)
        L = 8
        n = a.keys_per_gpu or 16 * M
        sh = D.weak_shard(rank, world, n)
        words = P.splitmix64_fill(SEED_KEYS, sh.first * L // 8, n * L // 8, device=dev)
        keys = words.view(torch.uint8).view(n, L)
        nr = 1024 if cfg == "records" else world
        ws = torch.empty(P.bucket_workspace_bytes(n, L, nr, records=True), dtype=torch.uint8, device=dev)
        kset = rot_copies(torch, keys)
        rsets = [P.bucket_records(k, nr, src_rank=rank, workspace=ws) for k in kset]
        bucketed = {"nranks": nr, "records": True}
        turn = [0]
        rotation = {"key_copies": len(kset), "output_sets": len(rsets)}

        def step():
            j = turn[0] % len(kset)
            turn[0] += 1
            rec, offs_ = P.bucket_records(kset[j], nr, src_rank=rank, out=rsets[j], workspace=ws)
            bucketed.update(rec=rec, offs=offs_)
            if cfg == "xrecords" and dist.is_initialized():
                bucketed["x"] = D.exchange_records(rec, offs_)
        out = None
        bytes_per_key = L + P.bucket_record_bytes(L)
        workload = (f"{cfg}: destination bucketing of {n >> 20}M x 8B keys per GPU by CityHash64 % {nr} into "
                    f"message_t wire records" + (" + all-to-all(v) exchange" if cfg == "xrecords" else ""))
        total_bytes_in = n * L
    elif cfg in ("bucket", "bucket8k", "exchange"):
        # f4: stable counting sort of 8-B keys by destination rank (keys, mbits,
        # ptindex, original index written at bucketed positions); "exchange"
        # buckets by the world size and ships each bucket to its owner with
        # all-to-all(v) (RCCL), inside the timed step
        L = 8
        n = a.keys_per_gpu or 16 * M
        sh = D.weak_shard(rank, world, n)
        words = P.splitmix64_fill(SEED_KEYS, sh.first * L // 8, n * L // 8, device=dev)
        keys = words.view(torch.uint8).view(n, L)
        nr = {"bucket": 1024, "bucket8k": 8192}.get(cfg, world)
        bucketed = {"nranks": nr}
        ws = torch.empty(P.bucket_workspace_bytes(n, L, nr), dtype=torch.uint8, device=dev)
        kset = rot_copies(torch, keys)
        bsets = [P.bucket_batch(k, 3, nr, with_ptindex=cfg != "exchange", workspace=ws) for k in kset]
        turn = [0]
        rotation = {"key_copies": len(kset), "output_sets": len(bsets)}

        def step():
            j = turn[0] % len(kset)
            turn[0] += 1
            ko, mb, pt, ix, offs_ = P.bucket_batch(kset[j], 3, nr, out=bsets[j], workspace=ws)
            bucketed.update(ko=ko, mb=mb, pt=pt, ix=ix, offs=offs_)
            if cfg == "exchange" and dist.is_initialized():
                bucketed["x"] = D.exchange_buckets(ko, mb, offs_, (ix.long() & 0xFFFFFFFF) + sh.first)
        out = None
        bytes_per_key = L + L + 8 + 4 + (4 if cfg != "exchange" else 0)
        workload = (f"{cfg}: destination bucketing of {n >> 20}M x 8B keys per GPU by "
                    f"CityHash64 % {nr}" + (" + all-to-all(v) exchange" if cfg == "exchange" else ""))
        total_bytes_in = n * L
    elif cfg == "cfg1":
        # BASELINE configs[0]: 1M x 64 B keys through hash.c (CityHash64 +
        # ptindex + rank); on the GPU: the fused placement batch (nptes 1 =
        # PDHT_DEFAULT_NUM_PTES, pdht_impl.h:41; 4 ranks as in README.txt:22)
        L = 64
        n = a.keys_per_gpu or M
        sh = D.weak_shard(rank, world, n)
        words = P.splitmix64_fill(SEED_KEYS, sh.first * L // 8, n * L // 8, device=dev)
        keys = words.view(torch.uint8).view(n, L)
        hist = torch.zeros(4, dtype=torch.int64, device=dev)
        # a 15-us launch: the step is the C call a C caller makes per batch
        # (pdht_place_batch_dev, checks and pointer lookups bound once), so
        # that the Python mirror's per-call cost does not set the step time
        kset = rot_copies(torch, keys)
        calls = []
        outs = None
        for k in kset:
            c, outs = P.bind_place_batch(k, 1, 4, hist=hist, out=outs)
            calls.append(c)
        turn = [0]
        rotation = {"key_copies": len(kset), "output_sets": 1}

        def step():
            calls[turn[0] % len(calls)]()
            turn[0] += 1
        out = outs[0]
        bytes_per_key = 64 + 8 + 4 + 4
        workload = f"cfg1: pdht_hash placement (mbits+ptindex+rank+hist) of {n >> 20}M x 64B keys per GPU"
        total_bytes_in = n * L
    elif cfg in ("cfg2", "cfg2r", "cfg4", "cfg5", "config4", "place"):
        L = 8 if cfg == "place" else 64
        n = a.keys_per_gpu or (128 * M if cfg == "cfg5" else 16 * M)
        sh = D.weak_shard(rank, world, n)
        if cfg == "config4":  # the 1B keys split over the ranks (strong scaling)
            sh = D.strong_shard(rank, world, CONFIG4_KEYS)
            n = sh.n
        words = P.splitmix64_fill(SEED_KEYS, sh.first * L // 8, n * L // 8, device=dev)
        keys = words.view(torch.uint8).view(n, L)
        if cfg == "cfg2r":
            # cfg2 with the digests written round-robin into 4 buffers (4 x 128
            # MiB): between two writes of one buffer 4 GiB of keys and 384 MiB
            # of other digests pass, so no digest line can wait in the 256 MiB
            # Infinity Cache for its next overwrite -- every step's digests
            # reach HBM, as cfg5's 1 GiB of digests must
            import itertools
            rot = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
            turn = itertools.cycle(range(4))
            out = rot[0]
            step = lambda: P.city64_batch(keys, out=rot[next(turn)])  # noqa: E731
            bytes_per_key = 64 + 8
            workload = (f"cfg2r: CityHash64 over {n >> 20}M x 64B keys per GPU, device-resident, digests written "
                        f"round-robin into 4 buffers (every step's digests reach HBM)")
        elif cfg in ("cfg2", "cfg5", "config4"):
            out = torch.empty(n, dtype=torch.int64, device=dev)
            step = lambda: P.city64_batch(keys, out=out)  # noqa: E731
            bytes_per_key = 64 + 8
            workload = (f"{cfg}: CityHash64 over {n >> 20}M x 64B keys per GPU, device-resident"
                        + (" (BASELINE configs[4] = 1B keys at N=8)" if cfg == "cfg5" else "")
                        + (f" (BASELINE configs[4]: 1B keys split over {world} GPU(s))" if cfg == "config4" else ""))
        elif cfg == "cfg4":
            out = torch.empty((n, 2), dtype=torch.int64, device=dev)
            step = lambda: P.citycrc128_batch(keys, out=out)  # noqa: E731
            bytes_per_key = 64 + 16
            workload = f"cfg4: CityHashCrc128 over {n >> 20}M x 64B keys per GPU, device-resident"
        else:
            hist = torch.zeros(1024, dtype=torch.int64, device=dev)
            outs = P.place_batch(keys, 3, 1024, hist=hist)
            out = outs[0]
            kset = rot_copies(torch, keys)
            turn = [0]
            rotation = {"key_copies": len(kset), "output_sets": 1}

            def step():
                P.place_batch(kset[turn[0] % len(kset)], 3, 1024, hist=hist, out=outs)
                turn[0] += 1
            bytes_per_key = 8 + 8 + 4 + 4
            workload = f"place: fused pdht_hash (mbits+ptindex+rank+hist) over {n >> 20}M x 8B keys per GPU"
        total_bytes_in = n * L
    elif cfg == "long":
        # f3: CityHashCrc128 above 900 B (CityHashCrc256 rounds, CRC-32C tables
        # in LDS) over 1M x 1 KiB keys, device-resident
        L = 1024
        n = a.keys_per_gpu or M
        sh = D.weak_shard(rank, world, n)
        words = P.splitmix64_fill(SEED_KEYS, sh.first * L // 8, n * L // 8, device=dev)
        keys = words.view(torch.uint8).view(n, L)
        out = torch.empty((n, 2), dtype=torch.int64, device=dev)
        step = lambda: P.citycrc128_batch(keys, out=out)  # noqa: E731
        bytes_per_key = L + 16
        workload = f"long: CityHashCrc128 over {n >> 20}M x 1KiB keys per GPU (CRC-32C path), device-resident"
        total_bytes_in = n * L
    else:  # cfg3 mixed lengths
        L = None
        n = a.keys_per_gpu or 64 * M
        sh = D.weak_shard(rank, world, n)
        lens = P.mixed_lengths(SEED_LENS, sh.first, n, 16, 256, device=dev)
        offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offs[1:])
        total = int(offs[-1].item())
        del lens
        # rank 0 hashes the canonical cfg3 byte stream (golden-checked); rank r
        # takes a disjoint segment of the same splitmix64 stream
        words = P.splitmix64_fill(SEED_KEYS, rank << 40, (total + 7) // 8 + 2, device=dev)
        data = words.view(torch.uint8)[:total]
        out = torch.empty(n, dtype=torch.int64, device=dev)
        P.city64_var_batch(data, offs, out=out)  # offsets bounds-checked once ...
        step = lambda: P.city64_var_batch(data, offs, out=out, check=False)  # noqa: E731  ... not per step
        bytes_per_key = total / n + 8 + 8
        total_bytes_in = total
        workload = f"cfg3: CityHash64 over {n >> 20}M mixed 16..256B keys per GPU (offset-indexed)"
    torch.cuda.synchronize()

    # ------------------------------------------------------------ timing ---
    for _ in range(a.warmup):
        step()
    kernel_name = P.last_kernel()
    torch.cuda.synchronize()
    flush_infinity_cache(torch, dev)
    # One event pair around the K steps, on the stream the kernels are launched
    # on: the launches queue back to back as a pipelined caller's would.
    # (r01-r03 bracketed every step with its own pair; on a 15-us launch
    # (cfg1) the two records per step outlasted the kernel, so the GPU idled
    # between steps waiting for the host and the per-step pairs timed that.)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(a.steps):
        step()
    ev1.record()
    torch.cuda.synchronize()
    D.barrier()
    elapsed = time.perf_counter() - t0
    kern_ms = ev0.elapsed_time(ev1) / a.steps
    elapsed_max, kern_ms_max = D.allreduce_max([elapsed, kern_ms], device=cdev)

    # what the last timed step handed its caller, before any other leg runs
    # (cfg1's wrapper leg and the parity call write the same buffers again)
    dumped = None
    if a.dump_outputs:
        if bucketed is not None:
            last = {k: bucketed.get(k) for k in ("rec", "ko", "mb", "pt", "ix", "offs")}
            last.update({f"x{i}": t for i, t in enumerate(bucketed.get("x", ()))})
            names = {"rec": "records", "ko": "keys_out", "mb": "mbits", "pt": "ptindex", "ix": "index",
                     "offs": "offsets", "x0": "exchanged_0", "x1": "exchanged_1", "x2": "exchanged_2",
                     "x3": "exchanged_3"}
            last = {names[k]: t for k, t in last.items()}
        elif cfg in ("cfg1", "place"):
            last = {"mbits": outs[0], "ptindex": outs[1], "rank": outs[2], "hist": hist}
        elif cfg == "cfg2r":  # the buffer the last step wrote (next(turn) is the one after it)
            last = {"digests": rot[(next(turn) - 1) % len(rot)]}
        else:
            last = {"digests": out}
        dumped = dump_outputs(torch, a.dump_outputs, last, rank)

    # cfg1's step is the bound C call; the Python mirror's place_batch (its
    # checks and pointer lookups on every call) timed the same way beside it
    wrapper = None
    if cfg == "cfg1" and a.full:
        wturn = [0]

        def wstep():
            P.place_batch(kset[wturn[0] % len(kset)], 1, 4, hist=hist, out=outs)
            wturn[0] += 1
        for _ in range(a.warmup):
            wstep()
        w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0w = time.perf_counter()
        w0.record()
        for _ in range(a.steps):
            wstep()
        w1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0w) / a.steps
        wms = w0.elapsed_time(w1) / a.steps
        wrapper = {"path": "pdht_amd.place_batch (Python wrapper, checks per call)",
                   "event_ms_per_step": round(wms, 4), "wall_ms_per_step": round(wall * 1e3, 4),
                   "Gkeys_s": round(n / max(wall, wms / 1e3) / 1e9, 4)}

    # -------------------------------------------- achievable read stream ---
    calib = None
    if keys is not None and a.full:
        P.read_stream(keys, True)
        cev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(10)]
        for s, e in cev:
            s.record()
            P.read_stream(keys, True)
            e.record()
        torch.cuda.synchronize()
        cms = float(np.median([s.elapsed_time(e) for s, e in cev]))
        calib = round(keys.numel() / (cms / 1e3) / 1e9, 1)
    # the 64-B kernel's own data movement with the hash replaced by an XOR fold
    calib_key = None
    if not a.full:
        pass
    elif cfg in ("cfg2", "cfg2r", "cfg5", "config4"):
        fold = torch.empty(n, dtype=torch.int64, device=dev)
        P.key_stream(keys, out=fold)
        cev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(10)]
        for s, e in cev:
            s.record()
            P.key_stream(keys, out=fold)
            e.record()
        torch.cuda.synchronize()
        cms = float(np.median([s.elapsed_time(e) for s, e in cev]))
        calib_key = round(bytes_per_key * n / (cms / 1e3) / 1e9, 1)
        del fold
    elif cfg == "cfg3":
        fold = torch.empty(n, dtype=torch.int64, device=dev)
        P.key_stream_var(data, offs, out=fold)
        cev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(5)]
        for s, e in cev:
            s.record()
            P.key_stream_var(data, offs, out=fold, check=False)
            e.record()
        torch.cuda.synchronize()
        cms = float(np.median([s.elapsed_time(e) for s, e in cev]))
        calib_key = round(bytes_per_key * n / (cms / 1e3) / 1e9, 1)
        del fold

    # ------------------------------------------------------------ parity ---
    if not a.full:
        parity = None
    elif bucketed is not None and bucketed.get("records"):
        parity = check_records(P, torch, D, sh, keys, bucketed, dev, cdev)
    elif bucketed is not None:
        parity = check_buckets(P, torch, D, sh, keys, bucketed, dev, cdev)
    else:
        extra = None
        if cfg in ("place", "cfg1"):  # one fresh call: the timed ones accumulated into hist
            hist.zero_()
            extra = (*P.place_batch(keys, *((1, 4) if cfg == "cfg1" else (3, 1024)), hist=hist), hist)
        if cfg == "cfg2r":
            ps = [check_parity(P, torch, D, "cfg2", sh, r, None, cdev) for r in rot]
            worst = min(ps, key=lambda p: list(PAR_WORD.values()).index(parity_word(p)))
            parity = worst + f" (all {len(rot)} rotating digest buffers)"
        else:
            parity = check_parity(P, torch, D, cfg, sh, out, extra, cdev)

    # ------------------------------------------------------- report ------
    value = (CONFIG4_KEYS if cfg == "config4" else n * world) * a.steps / elapsed_max / 1e9
    achieved = bytes_per_key * n / (kern_ms / 1e3) / 1e9
    res = {
        "metric": METRIC if cfg in ("cfg2", "cfg5", "cfg2r", "config4") else f"{cfg}: Gkeys/s and achieved HBM GB/s",
        "value": round(value, 4),
        "unit": "Gkeys/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(elapsed_max / a.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "strong" if cfg == "config4" else "weak",
        "vs_baseline": None,
        "dtype": "u64",
        "data": "synthetic: splitmix64 key bytes (seed 0x5EED5EED5EED5EED), generated on device",
        "config": {"workload": workload, "keys_per_gpu": n, "key_bytes": L,
                   "bytes_per_key": round(bytes_per_key, 3), "kernel": kernel_name,
                   "parallelism": f"{world} independent shards, no collective on the data path",
                   **({"rotation": dict(rotation, why="inputs below the 256 MiB Infinity Cache: steps cycle "
                                        "through copies so every step reads HBM")} if rotation else {})},
        "hbm_GBps": round(achieved * world, 1),
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": PEAK_HBM_GBPS,
                     "unit": "GB/s", "frac": round(achieved / PEAK_HBM_GBPS, 4),
                     "traffic": load_traffic(cfg, n, kernel_name), "kernel": kernel_name,
                     "event_ms_per_step": round(kern_ms, 4),
                     "event_ms_per_step_max_rank": round(kern_ms_max, 4),
                     "timing": "one HIP-event pair on the launch stream around the K back-to-back steps, / K "
                               "(includes any gap between launches; rocprofv3 kernel averages in profiles/)",
                     "read_only_GBps": round(total_bytes_in / (kern_ms / 1e3) / 1e9, 1),
                     "calibrated_read_stream_GBps": calib,
                     "calibrated_key_stream_GBps": calib_key},
        "full": a.full,
        **({"parity": parity} if a.full else {}),
    }
    if dumped is not None:
        res["dumped_outputs"] = dumped
    if wrapper is not None:
        res["cfg1_wrapper_path"] = wrapper
    if a.full and (world > 1 or dist.is_initialized()):
        res["per_rank"] = D.per_rank_report(rank, local, world, n, bytes_per_key, kern_ms, elapsed, a.steps,
                                            PEAK_HBM_GBPS, device=dev)
    if a.full and cfg in ("cfg2", "cfg3", "cfg4", "cfg5", "cfg1") and not a.no_host:  # (cfg2r: the host path of cfg2)
        hr = host_rate(P, torch, n, cfg, D, dev, cdev, var=(data, offs, out) if cfg == "cfg3" else None)
        if rank == 0:
            res["host_resident"] = hr
    if a.full and not a.no_cpu_baseline:
        # The reference city.c on this node's host cores, in the same run at
        # every N: rank 0 alone, after every rank's GPU leg has finished and
        # while the others sleep in a blocking (gloo) barrier, so no rank is
        # hashing or spinning on a core meanwhile.  Keys 0.. of the stream are
        # rank 0's shard at every N, so its GPU digests still check the sample.
        cpu_wait = None
        if world > 1:
            cpu_wait = dist.new_group(backend="gloo") if backend == "nccl" else dist.group.WORLD
            torch.cuda.synchronize()
            dist.barrier(group=cpu_wait)
        if rank == 0:
            res["cpu_baseline"] = cpu_baseline(cfg, a.cpu_seconds, out, P, torch)
            if world > 1:
                res["cpu_baseline"]["while"] = (f"rank 0 of {world}, after every rank's GPU leg; the other "
                                                f"{world - 1} ranks blocked in a gloo barrier")
        if cpu_wait is not None:
            dist.barrier(group=cpu_wait)
    if "config4" in plan(a, world):
        del keys, out, words
        kset = rsets = bsets = calls = None  # noqa: F841 (free the rotation copies)
        torch.cuda.empty_cache()
        c4 = config4_block(P, torch, D, a, rank, local, world, dev, cdev)
        if rank == 0:
            res["baseline_config4"] = c4
            # the line leads with the worse of the two words (FAILED < unchecked < ok)
            order = list(PAR_WORD.values())
            w4, w0 = parity_word(c4["parity"]), parity_word(res["parity"])
            if order.index(w4) < order.index(w0):
                res["parity"] = f"{w4}: " + res["parity"] + " | configs[4] block: " + c4["parity"]
    if rank == 0:
        print(json.dumps(res), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


def config4_block(P, torch, D, a, rank, local, world, dev, cdev) -> dict:
    """BASELINE configs[4] at this world size: the 1B x 64 B key stream split
    contiguously over the N ranks (strong scaling, pdht_amd.dist.strong_shard;
    the reference places keys the same way, each SPMD rank hashing its own,
    README.txt:20-22, libpdht/hash.c:29), keys generated in HBM, CityHash64
    in ~512 MiB launches.  Timed as the main leg (barrier + synchronize on both
    sides of K back-to-back steps, max over ranks) and checked bit-exact: each
    rank's fold of its slice against the sum of the committed reference folds
    of the 16M-key chunks it covers."""
    sh = D.strong_shard(rank, world, CONFIG4_KEYS)
    words = P.splitmix64_fill(SEED_KEYS, sh.first * 8, sh.n * 8, device=dev)
    keys = words.view(torch.uint8).view(sh.n, 64)
    out = torch.empty(sh.n, dtype=torch.int64, device=dev)
    for _ in range(max(1, a.warmup // 5)):
        P.city64_batch(keys, out=out)
    steps = max(3, a.steps // 5)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    flush_infinity_cache(torch, dev)
    torch.cuda.synchronize()
    D.barrier()
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(steps):
        P.city64_batch(keys, out=out)
    ev1.record()
    torch.cuda.synchronize()
    D.barrier()
    elapsed = time.perf_counter() - t0
    ev_ms = ev0.elapsed_time(ev1) / steps
    elapsed_max = D.allreduce_max([elapsed], device=cdev)[0]
    kernel = P.last_kernel()
    want = city64_chunk_fold(golden_folds(), sh.first, sh.n)
    if want is None:
        st, msg = PAR_UNCHECKED, f"rank {rank}: no reference fold for keys {sh.first}..+{sh.n}"
    else:
        good = D.fold_tensor(out, sh.first) == want
        st = PAR_OK if good else PAR_FAIL
        msg = (f"rank {rank}: fold of keys {sh.first}..+{sh.n} {'==' if good else '!='} reference golden "
               f"(16M-key chunks {sh.first >> 24}..{((sh.first + sh.n) >> 24) - 1})")
    parity = combine_parity(D, st, [msg], world, cdev)
    pr = D.per_rank_report(rank, local, world, sh.n, 72.0, ev_ms, elapsed,
                           steps, PEAK_HBM_GBPS, device=dev)
    value = CONFIG4_KEYS * steps / elapsed_max / 1e9
    del keys, out, words
    torch.cuda.empty_cache()
    return {"workload": "BASELINE configs[4]: 1B x 64B keys (CityHash64) split over the N GPUs, device-resident",
            "keys_total": CONFIG4_KEYS,
            "scaling": "strong", "steps": steps, "ms_per_step": round(elapsed_max / steps * 1e3, 4),
            "value": round(value, 4), "unit": "Gkeys/s", "kernel": kernel,
            "keys_per_gpu": [r["keys"] for r in pr["ranks"]],
            "aggregate_frac": round(CONFIG4_KEYS * 72.0 / (elapsed_max / steps) / 1e9 / (world * PEAK_HBM_GBPS), 4),
            "per_gpu_Gkeys_s": pr["Gkeys_s"], "per_gpu_frac": pr["frac"],
            "per_gpu_event_ms": [r["event_ms"] for r in pr["ranks"]],
            "parity": parity}


def load_traffic(cfg, n, kernel):
    """HBM bytes per launch from the committed rocprofv3 PMC passes, only if
    they were taken of exactly the kernel (and launch shape) that ran here."""
    p = os.path.join(ROOT, "profiles", f"traffic_{cfg}.json")
    if not os.path.exists(p):
        return None
    try:
        with open(p) as f:
            t = json.load(f)
        if int(t.get("keys_per_launch", -1)) != n or t.get("kernel_tag") != kernel:
            return None
        return t.get("hbm_bytes_per_launch")
    except Exception:
        return None


def city64_chunk_fold(folds, first, n):
    """Reference fold of keys [first, first+n) of the 64-B key stream, summed
    from the committed 16M-key chunk folds of the 1B-key config (the fold is
    position-weighted by global index, so chunk folds add); None when the
    range is not made of whole chunks inside the 1B keys."""
    c5 = (folds or {}).get("cfg5_city64_1B_x64", {})
    ch, ck = c5.get("chunks"), int(c5.get("chunk_keys", 16 * M))
    if not ch or n <= 0 or first % ck or n % ck or (first + n) // ck > len(ch):
        return None
    return sum(int(ch[j], 16) for j in range(first // ck, (first + n) // ck)) & ((1 << 64) - 1)


def golden_shard_fold(folds, cfg, sh):
    """Reference fold of exactly this shard's keys, when the golden file has it."""
    if folds is None:
        return None, None
    if cfg in ("cfg2", "cfg5", "config4"):
        f = city64_chunk_fold(folds, sh.first, sh.n)
        if f is not None:
            return f, f"cfg5 16M-key chunks {sh.first // (16 * M)}..{(sh.first + sh.n) // (16 * M) - 1}"
    if cfg == "long" and sh.n == M and sh.first % M == 0:
        g = folds.get("long_crc128_1M_x1024", {}).get("shards", [])
        if sh.first // M < len(g):
            return int(g[sh.first // M], 16), f"long shard {sh.first // M}"
    if cfg == "cfg4" and sh.n == 16 * M and sh.first % (16 * M) == 0:
        c4 = folds.get("cfg4_crc128_16M_x64", {})
        r = sh.first // (16 * M)
        if r == 0:
            return int(c4["total"], 16), "cfg4 total"
        if r < len(c4.get("rank_chunks", [])):
            return int(c4["rank_chunks"][r], 16), f"cfg4 weak shard {r}"
    if cfg == "cfg3" and sh.n == 64 * M and sh.first == sh.rank * 64 * M:
        c3 = folds.get("cfg3_city64_64M_mixed", {})
        if sh.rank == 0:
            return int(c3["total"], 16), "cfg3 total"
        if sh.rank < len(c3.get("ranks", [])):
            return int(c3["ranks"][sh.rank]["fold"], 16), f"cfg3 rank {sh.rank}"
    return None, None


# parity status of one shard, combined over ranks by MIN: any failure makes the
# line FAILED, any shard without a reference fold makes it "unchecked"
PAR_FAIL, PAR_UNCHECKED, PAR_OK = 0, 1, 2
PAR_WORD = {PAR_FAIL: "FAILED", PAR_UNCHECKED: "unchecked", PAR_OK: "ok"}


def parity_word(p: str) -> str:
    """"ok" / "unchecked" / "FAILED": the first word of a parity string."""
    return p.split()[0].rstrip(":")


def combine_parity(D, status, msgs, world, cdev):
    """One parity string for the whole job: the worst status over ranks, and
    every rank's own finding (gathered, in rank order)."""
    worst = D.allreduce_min_int(status, device=cdev)
    if world > 1:
        import torch.distributed as dist
        allm = [None] * world
        dist.all_gather_object(allm, f"[rank {dist.get_rank()}: {PAR_WORD[status]}] " + "; ".join(msgs))
        return f"{PAR_WORD[worst]} (worst of {world} ranks): " + " ".join(allm)
    return f"{PAR_WORD[worst]}: " + "; ".join(msgs)


def check_parity(P, torch, D, cfg, sh, out, extra, cdev):
    """Bit-exact check of this rank's WHOLE shard against the reference golden
    folds (tests/golden/config_folds.json: data generated from the reference
    city.c by tests/golden/gen_golden.py).  A shard the golden file has no
    fold for is reported "unchecked", never "ok".  No oracle code runs here;
    the cpu_baseline leg separately compares the reference's own digests of
    its sample with this run's GPU digests."""
    folds = golden_folds()
    if folds is None:
        return combine_parity(D, PAR_UNCHECKED, ["tests/golden/config_folds.json missing"], sh.world, cdev)
    msgs, st = [], PAR_UNCHECKED
    if cfg in ("cfg1", "place"):
        want = None
        if cfg == "cfg1":
            f = folds.get("cfg1_pdht_hash_1M_x64", {})
            pl = [x for x in f.get("placements", []) if x["nptes"] == 1 and x["nranks"] == 4]
            r = sh.first // M
            if sh.n == f.get("n") and sh.first % M == 0 and pl:
                if r == 0:
                    want = {"mbits": f["mbits"], "ptindex": pl[0]["ptindex"], "rank": pl[0]["rank"],
                            "hist": pl[0]["hist"]}
                elif r < len(f.get("ranks", [])):
                    want = f["ranks"][r]
            what = f"cfg1 rank {r}, nptes 1, nranks 4"
        else:
            r = sh.first // (16 * M)
            g = folds.get("place_8B_16M", {}).get("shards", [])
            if sh.n == 16 * M and sh.first % (16 * M) == 0 and r < len(g):
                want = g[r]
            what = f"place shard {r}"
        if want is not None:
            mb, pt, rk, hist = extra
            got = {"mbits": D.fold_tensor(mb, sh.first),
                   "ptindex": D.fold_tensor(pt.to(torch.int64) & 0xFFFFFFFF, sh.first),
                   "rank": D.fold_tensor(rk.to(torch.int64) & 0xFFFFFFFF, sh.first),
                   "hist": D.fold_tensor(hist, 0)}
            bad = [k for k, v in got.items() if v != int(want[k], 16)]
            st = PAR_FAIL if bad else PAR_OK
            msgs.append(f"mbits, ptindex, rank and histogram folds {'!=' if bad else '=='} reference golden "
                        f"({what})" + (f" (mismatch: {bad})" if bad else ""))
        else:
            msgs.append(f"rank {sh.rank}: no reference fold for keys {sh.first}..+{sh.n}")
    else:
        want, what = golden_shard_fold(folds, cfg, sh)
        if want is not None:
            first_idx = 2 * sh.first if cfg in ("cfg4", "long") else sh.first
            good = D.fold_tensor(out, first_idx) == want
            st = PAR_OK if good else PAR_FAIL
            msgs.append(f"full-shard fold {'==' if good else '!='} reference golden ({what})")
        else:
            msgs.append(f"rank {sh.rank}: no reference fold for keys {sh.first}..+{sh.n}")
    return combine_parity(D, st, msgs, sh.world, cdev)


def check_buckets(P, torch, D, sh, keys, b, dev, cdev):
    """Bucketing checks without oracle code: the whole shard's bucketed mbits,
    original indices and bucket offsets against the reference golden folds
    (bucket config), and full-size properties on the device -- index is a
    permutation, ranks are non-decreasing, indices increase inside a bucket,
    keys_out == keys[index], mbits == CityHash64(keys_out)."""
    nr, ko, mb, ix, offs = b["nranks"], b["ko"], b["mb"], b["ix"], b["offs"]
    n = ix.numel()
    msgs, ok, golden = [], True, False
    folds = golden_folds() or {}
    g = folds.get("bucket_8B_16M" if nr == 1024 else f"bucket_8B_16M_{nr}", {})
    r = sh.first // (16 * M)
    if nr == g.get("nranks") and n == g.get("n") and sh.first % n == 0 and r < len(g.get("shards", [])):
        gs = g["shards"][r]
        got = {"mbits": D.fold_tensor(mb, 0), "index": D.fold_tensor(ix, 0), "offsets": D.fold_tensor(offs, 0)}
        bad = [k for k, v in got.items() if v != int(gs[k], 16)]
        ok, golden = not bad, True
        msgs.append(f"bucketed mbits, index and offsets folds {'==' if ok else '!='} reference golden "
                    f"(bucket shard {r})" + (f" (mismatch: {bad})" if bad else ""))
    else:
        msgs.append(f"rank {sh.rank}: no reference fold for this bucketing (properties only)")
    ix = ix.long() & 0xFFFFFFFF
    srt = torch.sort(ix).values
    perm = bool((srt == torch.arange(n, device=dev)).all().item())
    same = bool((ko == keys[ix]).all().item()) and bool((P.city64_batch(ko) == mb).all().item())
    cnt = (offs[1:] - offs[:-1])
    rk = torch.repeat_interleave(torch.arange(nr, device=dev), cnt)
    prop = perm and same and int(offs[-1].item()) == n
    if n > 1:
        prop = prop and bool(((ix[1:] > ix[:-1]) | (rk[1:] > rk[:-1])).all().item())
    msgs.append(f"full batch: permutation, stable buckets, keys/mbits consistent {'ok' if prop else 'FAILED'}")
    ok = ok and prop
    if "x" in b:
        xk, xm, xi, _ = b["x"]
        got_m = xm.cpu().numpy().view(np.uint64)
        mine = bool((got_m % np.uint64(sh.world) == np.uint64(sh.rank)).all())
        mine = mine and bool((P.city64_batch(xk) == xm).all().item())
        # received key j is global key xi[j]: regenerate it with the device
        # generator (pinned to the oracle by tests/test_gpu_parity.py)
        for j in range(0, xi.numel(), max(1, xi.numel() // 256)):
            want = P.splitmix64_fill(SEED_KEYS, int(xi[j].item()), 1, device=dev)
            mine = mine and bool((xk[j].view(torch.int64) == want).all().item())
        msgs.append(f"exchange: {xi.numel()} keys received, all owned by this rank {'ok' if mine else 'FAILED'}")
        ok = ok and mine
    st = PAR_FAIL if not ok else (PAR_OK if golden else PAR_UNCHECKED)
    return combine_parity(D, st, msgs, sh.world, cdev)


def check_records(P, torch, D, sh, keys, b, dev, cdev):
    """Record bucketing checks without oracle code: the records' mbits and
    source-index columns and the bucket offsets against the same reference
    golden folds as the array form (bucket config), and full-size properties:
    index is a permutation, buckets are stable, every record's key and mbits
    agree with the keys at its source index and with CityHash64 of its key."""
    nr, rec, offs = b["nranks"], b["rec"], b["offs"]
    n = rec.shape[0]
    ty, sr, hi, ix32, mb, ko = P.record_fields(rec, keys.shape[1])
    ix = ix32.to(torch.int64) & 0xFFFFFFFF
    msgs, ok, golden = [], True, False
    folds = golden_folds() or {}
    g = folds.get("bucket_8B_16M" if nr == 1024 else f"bucket_8B_16M_{nr}", {})
    r = sh.first // (16 * M)
    if nr == g.get("nranks") and n == g.get("n") and sh.first % n == 0 and r < len(g.get("shards", [])):
        gs = g["shards"][r]
        got = {"mbits": D.fold_tensor(mb, 0), "index": D.fold_tensor(ix, 0), "offsets": D.fold_tensor(offs, 0)}
        bad = [k for k, v in got.items() if v != int(gs[k], 16)]
        ok, golden = not bad, True
        msgs.append(f"records' mbits, index and offsets folds {'==' if ok else '!='} reference golden "
                    f"(bucket shard {r})" + (f" (mismatch: {bad})" if bad else ""))
    else:
        msgs.append(f"rank {sh.rank}: no reference fold for this bucketing (properties only)")
    perm = bool((torch.sort(ix).values == torch.arange(n, device=dev)).all().item())
    same = bool((ko == keys[ix]).all().item()) and bool((P.city64_batch(ko.contiguous()) == mb).all().item())
    hdr = bool(((ty == P.PDHT_PUT) & (sr == sh.rank) & (hi == 0)).all().item())
    cnt = offs[1:] - offs[:-1]
    rk = torch.repeat_interleave(torch.arange(nr, device=dev), cnt)
    prop = perm and same and hdr and int(offs[-1].item()) == n
    if n > 1:
        prop = prop and bool(((ix[1:] > ix[:-1]) | (rk[1:] > rk[:-1])).all().item())
    msgs.append(f"full batch: permutation, stable buckets, headers, keys/mbits consistent {'ok' if prop else 'FAILED'}")
    ok = ok and prop
    if "x" in b:
        xr, _ = b["x"]
        xt, xs, xh, xi, xm, xk = P.record_fields(xr, keys.shape[1])
        got_m = xm.cpu().numpy().view(np.uint64)
        mine = bool((got_m % np.uint64(sh.world) == np.uint64(sh.rank)).all())
        mine = mine and bool((P.city64_batch(xk.contiguous()) == xm).all().item())
        gidx = xs.to(torch.int64) * sh.n + (xi.to(torch.int64) & 0xFFFFFFFF)
        for j in range(0, gidx.numel(), max(1, gidx.numel() // 256)):
            want = P.splitmix64_fill(SEED_KEYS, int(gidx[j].item()), 1, device=dev)
            mine = mine and bool((xk[j].contiguous().view(torch.int64) == want).all().item())
        msgs.append(f"exchange: {xr.shape[0]} records received, all owned by this rank {'ok' if mine else 'FAILED'}")
        ok = ok and mine
    st = PAR_FAIL if not ok else (PAR_OK if golden else PAR_UNCHECKED)
    return combine_parity(D, st, msgs, sh.world, cdev)


def host_rate(P, torch, n, cfg, D, dev, cdev, var=None):
    """Host-resident rate: pinned keys in, pinned digests out, through the
    C-ABI host entry point (zero-copy for pinned buffers; PCIe-bound).  At
    N > 1 every rank runs at the same time on its own GPU (its own PCIe
    link): per-rank rates and the aggregate over the slowest rank.

    `var` = (bytes, offsets, digests) of cfg3's offset-indexed keys on the
    device: the first 16M keys (4M at N > 1) are copied into pinned host
    bytes + offsets, hashed through pdht_city64_batch_var_host, and the host
    digests compared with the device run's digests of the same keys (which
    the line's parity checks against the reference folds)."""
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    try:
        m = min(n, 16 * M if world == 1 else 4 * M)
        match = None
        if var is not None:
            vdata, voffs, vout = var
            nb = int(voffs[m].item())
            hdata = torch.empty(nb, dtype=torch.uint8).pin_memory()
            hdata.copy_(vdata[:nb])
            hoffs = torch.empty(m + 1, dtype=torch.int64).pin_memory()
            hoffs.copy_(voffs[:m + 1])
            out = torch.empty(m, dtype=torch.int64).pin_memory()
            out.fill_(0)
            bpk = nb / m + 8 + 8  # key bytes + offset + digest over PCIe

            def fn():
                P.city64_var_batch_host(hdata, hoffs, out=out, device=dev.index)
            fn()  # warm-up
            match = bool(torch.equal(out, vout[:m].cpu()))
        else:
            keys = torch.empty((m, 64), dtype=torch.uint8).pin_memory()
            keys.view(-1).view(torch.int64).copy_(
                P.splitmix64_fill(SEED_KEYS, rank * m * 8, m * 8, device=dev).cpu())
            w = 2 if cfg == "cfg4" else 1
            out = torch.empty((m, w) if w == 2 else (m,), dtype=torch.int64).pin_memory()
            hfn = P.citycrc128_batch_host if cfg == "cfg4" else P.city64_batch_host
            bpk = 64 + 8 * w

            def fn():
                hfn(keys, out=out, device=dev.index)
            fn()  # warm-up
        reps = 3
        D.barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        dt = (time.perf_counter() - t0) / reps
        D.barrier()
        mine = {"Gkeys_s": round(m / dt / 1e9, 4), "GBps_pcie": round(m * bpk / dt / 1e9, 2), "match": match}
        res = {"value": mine["Gkeys_s"], "unit": "Gkeys/s", "keys": m, "GBps_pcie": mine["GBps_pcie"],
               "note": "pinned host keys and digests; the kernel reads/writes them over PCIe (zero-copy)"}
        if var is not None:
            res["note"] = ("pinned host key bytes + u64 offsets (the first keys of this rank's cfg3 stream) and "
                           "pinned digests; the window kernel reads/writes them over PCIe (zero-copy)")
            res["key_bytes"] = nb
            res["digests_equal_device_run"] = match
        if world > 1:
            dtmax = D.allreduce_max([dt], device=cdev)[0]
            allr = [None] * world
            dist.all_gather_object(allr, mine)
            res.update(value=round(m * world / dtmax / 1e9, 4), keys=m * world,
                       per_rank_Gkeys_s=[r["Gkeys_s"] for r in allr],
                       per_rank_GBps_pcie=[r["GBps_pcie"] for r in allr],
                       note=res["note"] + f"; {world} GPUs at once, one PCIe link each; value = all keys / "
                                          "slowest rank")
            if var is not None:
                res["digests_equal_device_run"] = all(r["match"] for r in allr)
        return res
    except Exception as e:  # pragma: no cover
        return {"error": str(e)}


def host_cpus():
    """CPUs this job may use: the affinity set capped by the cgroup v2 CPU
    quota (a GPU box grants a share of a large host), plus the NUMA layout."""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = int(q) / int(per)
    except Exception:
        pass
    nodes = []
    base = "/sys/devices/system/node"
    if os.path.isdir(base):
        for d in sorted(os.listdir(base)):
            if d.startswith("node") and d[4:].isdigit():
                try:
                    nodes.append({"node": int(d[4:]), "cpus": open(f"{base}/{d}/cpulist").read().strip()})
                except OSError:
                    pass
    use = aff if quota is None else max(1, min(aff, int(quota)))
    return {"threads": use, "affinity_cpus": aff, "cgroup_quota_cpus": quota,
            "nproc_online": os.cpu_count(), "numa_nodes": nodes}


def cpu_baseline(cfg, budget_s: float, gpu_out, P, torch):
    """The reference city.c (oracle/_ref) on this host over a bounded sample
    of the same workload, as BASELINE.md §3 specifies:
      cfg1   one thread, per-key pdht_hash semantics (CityHash64 + hash.c:27
             and :29's two reductions) over all 1M x 64 B keys;
      others all the CPUs this job may use (host_cpus), contiguous slices;
      cfg4/long the -msse4.2 build's CityHashCrc128 (pdht.mk:21, city.c:402).
    Timer CLOCK_MONOTONIC_RAW (pdht_inline.h:33-41), one warm-up pass, then
    best of 5 timed passes, each repeating the sample to fill ~budget_s.  The
    reference's digests of its sample are compared with this run's GPU
    digests of the same keys."""
    from oracle import oracle as O
    cpus = host_cpus()
    thr = 1 if cfg == "cfg1" else cpus["threads"]
    mode, offsets, L = 0, None, 64
    fname = "CityHash64"
    nptes = nranks = 1
    if cfg == "cfg1":
        s_n, mode, nptes, nranks = M, 2, 1, 4
        data = O.fixed_keys(s_n, 64)
        what = "all 1M x 64B keys of cfg1, per-key pdht_hash semantics (nptes 1, nranks 4)"
    elif cfg in ("cfg2", "cfg2r", "cfg5", "config4"):
        s_n = 4 * M
        data = O.fixed_keys(s_n, 64)
        what = "the first 4M x 64B keys of the stream"
    elif cfg == "cfg4":
        s_n, mode, fname = 4 * M, 1, "CityHashCrc128"
        data = O.fixed_keys(s_n, 64)
        what = "the first 4M x 64B keys, CityHashCrc128 (-msse4.2 build)"
    elif cfg == "long":
        s_n, mode, fname, L = M // 4, 1, "CityHashCrc128", 1024
        data = O.fixed_keys(s_n, 1024)
        what = "the first 256K x 1KiB keys, CityHashCrc128 (CityHashCrc256 rounds, -msse4.2 build)"
    elif cfg == "cfg3":
        s_n = 4 * M
        data, offsets = O.mixed_keys(s_n)
        L = 0
        what = "the first 4M mixed 16..256B keys of the stream (offset-indexed)"
    elif cfg == "place":
        s_n, mode, nptes, nranks, L = 4 * M, 2, 3, 1024, 8
        data = O.fixed_keys(s_n, 8)
        what = f"the first 4M x 8B keys, pdht_hash semantics (nptes 3, nranks {nranks})"
    elif cfg in ("bucket", "bucket8k", "exchange", "records", "xrecords"):
        return cpu_bucket_baseline(cfg, budget_s, P, torch, O, cpus)
    else:
        return None
    try:
        fn, kind = O.cpu_fn(fname)
    except RuntimeError as e:
        return {"error": str(e)}

    outs = None

    def run(reps):
        return O.time_batch(mode, fn, data, s_n, offsets=offsets, L=L, threads=thr, reps=reps,
                            nptes=nptes, nranks=nranks, outs=outs)

    _, dig, pt_, rk_ = run(1)  # pages in the sample and the outputs
    outs = (dig, pt_, rk_)
    # warm-up: at least 1 s of the same work first (cores idling before the
    # run need about that long to reach their steady clock; measured here)
    t_w, secs = 0.0, float("inf")
    while t_w < 1.0:
        dt = run(1)[0]
        t_w += dt
        secs = min(secs, dt)
    reps = max(1, int(budget_s / max(secs, 1e-6)))
    best = min(run(reps)[0] for _ in range(5))
    ok = None
    if gpu_out is not None:
        g = gpu_out.reshape(-1)[: dig.size].cpu().numpy().view(np.uint64)
        if cfg == "cfg3" or cfg in ("cfg1", "cfg2", "cfg2r", "cfg4", "cfg5", "config4", "long", "place"):
            ok = bool((dig[: g.size] == g).all()) if g.size == dig.size else None
    res = {"value": round(s_n * reps / best / 1e9, 4), "unit": "Gkeys/s", "cores": thr, "kind": kind,
           "sample": f"{what}; {reps} passes per timing, best of 5 ({best:.2f} s wall, "
                     f"{best * thr:.1f} CPU-s)",
           "timer": "CLOCK_MONOTONIC_RAW", "host": cpus, "gpu_digests_equal_reference": ok}
    if cfg in ("cfg2", "cfg2r", "cfg5", "config4"):
        # BASELINE.md §3's other leg on the same box: one thread through
        # per-key pdht_hash over cfg1's 1M x 64 B keys
        k1 = O.fixed_keys(M, 64)
        _, d1, p1, r1 = O.time_batch(2, fn, k1, M, L=64, threads=1, reps=20, nptes=1, nranks=4)
        one = min(O.time_batch(2, fn, k1, M, L=64, threads=1, reps=1, nptes=1, nranks=4,
                               outs=(d1, p1, r1))[0] for _ in range(5))
        res["cfg1_single_thread_pdht_hash_Gkeys_s"] = round(M / one / 1e9, 4)
    return res


def cpu_bucket_baseline(cfg, budget_s, P, torch, O, cpus):
    """f4's CPU baseline: destination bucketing on the host cores -- the
    reference CityHash64 (oracle/_ref) per key, a count per rank and a stable
    scatter by rank (the count-then-ship shape of
    bench/Meraculous/buildUFXhashBinary.h:103-109, :255-279), with every
    thread of the job's CPU share (oracle_time_bucket).  Outputs as the GPU's:
    bucketed keys, mbits, ptindex and original index (records: the wire
    records).  Best of 5 after >= 1 s of warm-up; the sample's bucketing is
    compared with the GPU's bucketing of the same keys."""
    thr = cpus["threads"]
    s_n, L = 4 * M, 8
    records = cfg in ("records", "xrecords")
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    nranks = {"bucket": 1024, "bucket8k": 8192, "records": 1024}.get(cfg, world)
    keys = O.fixed_keys(s_n, L)
    try:
        fn, kind = O.cpu_fn("CityHash64")
    except RuntimeError as e:
        return {"error": str(e)}
    bufs = O.BucketBufs(s_n, L, nranks, thr, records)

    def run(reps):
        return O.time_bucket(fn, keys, 3, nranks, threads=thr, reps=reps, records=records, bufs=bufs)[0]

    run(1)
    t_w, secs = 0.0, float("inf")
    while t_w < 1.0:
        dt = run(1)
        t_w += dt
        secs = min(secs, dt)
    reps = max(1, int(budget_s / max(secs, 1e-6)))
    best = min(run(reps) for _ in range(5))
    # the GPU's bucketing of the same sample, compared field by field
    kd = torch.from_numpy(keys).to(torch.device("cuda", torch.cuda.current_device()))
    if records:
        rec, offs = P.bucket_records(kd, nranks)
        ok = bool((rec.cpu().numpy() == bufs.rec).all()) and bool((offs.cpu().numpy() == bufs.offsets.view(np.int64)).all())
    else:
        ko, mb, pt, ix, offs = P.bucket_batch(kd, 3, nranks)
        ok = (bool((ko.cpu().numpy() == bufs.keys).all()) and bool((mb.cpu().numpy().view(np.uint64) == bufs.mbits).all())
              and bool((pt.cpu().numpy().view(np.uint32) == bufs.pt).all())
              and bool((ix.cpu().numpy().view(np.uint32) == bufs.idx).all())
              and bool((offs.cpu().numpy() == bufs.offsets.view(np.int64)).all()))
    form = "wire records" if records else "keys, mbits, ptindex and index arrays"
    return {"value": round(s_n * reps / best / 1e9, 4), "unit": "Gkeys/s", "cores": thr,
            "kind": kind,
            "sample": (f"the first 4M x 8B keys bucketed by rank = CityHash64 % {nranks} into {form}: reference "
                       f"CityHash64 per key, a count per rank and a stable scatter by rank (the Meraculous "
                       f"count-then-ship shape, restated in oracle_time_bucket); {reps} bucketings per timing, "
                       f"best of 5 ({best:.2f} s wall, {best * thr:.1f} CPU-s)"),
            "timer": "CLOCK_MONOTONIC_RAW", "host": cpus, "gpu_digests_equal_reference": ok}


if __name__ == "__main__":
    main()
