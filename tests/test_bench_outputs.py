"""bench.py --dump-outputs and the plain / --full split of the line.

dump_outputs() stores every value exactly (a 64-bit integer as its high and
low 32 bits in float64), cuts a large array to the same seeded sample of rows
in every run and stays under 64 MB; a plain run prints the headline fields
and none of the --full legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _u64(a):
    """The uint64 column(s) back from a dump's (hi32, lo32) float64 pairs."""
    a = a.astype(np.uint64)
    return (a[:, 0::2] << np.uint64(32)) | a[:, 1::2]


def test_dump_is_exact_for_every_dtype(tmp_path):
    rng = np.random.default_rng(11)
    d64 = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    d64[:3] = [0, 2 ** 64 - 1, 2 ** 63]
    d128 = rng.integers(0, 2 ** 64, (500, 2), dtype=np.uint64)
    i32 = rng.integers(-2 ** 31, 2 ** 31, 777, dtype=np.int64).astype(np.int32)
    u8 = rng.integers(0, 256, (333, 8), dtype=np.uint8)
    info = bench.dump_outputs(torch, str(tmp_path), {
        "digests": torch.from_numpy(d64.view(np.int64)), "pairs": torch.from_numpy(d128.view(np.int64)),
        "ptindex": torch.from_numpy(i32), "keys_out": torch.from_numpy(u8), "absent": None})
    assert sorted(os.listdir(tmp_path)) == ["digests.npy", "keys_out.npy", "pairs.npy", "ptindex.npy"]
    got = {k: np.load(tmp_path / f"{k}.npy") for k in ("digests", "pairs", "ptindex", "keys_out")}
    assert got["digests"].dtype == np.float64 and got["digests"].shape == (1000, 2)
    assert (_u64(got["digests"])[:, 0] == d64).all()
    assert got["pairs"].shape == (500, 4) and (_u64(got["pairs"]) == d128).all()
    assert got["ptindex"].dtype == np.float64 and (got["ptindex"][:, 0] == i32).all()
    assert got["keys_out"].dtype == np.float32 and (got["keys_out"] == u8).all()
    assert info["bytes"] == sum(a.nbytes for a in got.values())
    assert info["arrays"]["digests"]["rows"] == info["arrays"]["digests"]["of"] == 1000


def test_large_arrays_are_cut_to_one_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 16)
    n = 100_003
    d = torch.arange(n, dtype=torch.int64) * 0x9E3779B97F4A7C15
    small = torch.arange(10, dtype=torch.int64)
    a = bench.dump_outputs(torch, str(tmp_path / "a"), {"digests": d, "offsets": small})
    b = bench.dump_outputs(torch, str(tmp_path / "b"), {"digests": d, "offsets": small}, rank=3)
    x, y = np.load(tmp_path / "a" / "digests.npy"), np.load(tmp_path / "b" / "digests.rank3.npy")
    assert (x == y).all() and a["bytes"] == b["bytes"] <= 1 << 16
    rows = x.shape[0]
    assert 2 <= rows <= (1 << 15) // 16 and a["arrays"]["digests"] == {"file": "digests.npy", "rows": rows,
                                                                       "of": n, "dtype": "float64"}
    # the sampled rows are rows of d in increasing order, the first and the last among them
    got = _u64(x)[:, 0].view(np.int64)
    idx = np.flatnonzero(np.isin(d.numpy(), got))
    assert idx.size == rows and idx[0] == 0 and idx[-1] == n - 1 and (d.numpy()[idx] == got).all()
    assert (_u64(np.load(tmp_path / "a" / "offsets.npy"))[:, 0] == np.arange(10)).all()  # small ones whole


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_digests(tmp_path):
    """A plain run of the flagship config (fewer keys): the line has the
    contract fields and ms_per_step and none of the --full legs, --steps sets
    the timed steps, and the dumped digests are CityHash64 of the same keys."""
    import pdht_amd as P
    n = 100_003
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--keys-per-gpu", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    (r,) = [json.loads(s) for s in p.stdout.splitlines() if s.startswith("{")]
    assert r["steps"] == 3 and r["warmup"] == 1 and r["full"] is False
    assert r["metric"] == bench.METRIC and r["unit"] == "Gkeys/s" and r["higher_is_better"] is True
    assert r["dtype"] == "u64" and r["ms_per_step"] > 0
    # value = keys / step time; both are printed rounded to 4 decimals (ms_per_step of ~0.01 ms: <= 0.5 %)
    assert abs(r["value"] - n / (r["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * r["value"]
    for leg in ("parity", "cpu_baseline", "host_resident", "baseline_config4", "per_rank", "cfg1_wrapper_path"):
        assert leg not in r, leg
    assert r["roofline"]["calibrated_read_stream_GBps"] is None
    assert os.listdir(tmp_path) == ["digests.npy"]
    dev = torch.device("cuda:0")
    keys = P.splitmix64_fill(bench.SEED_KEYS, 0, n * 8, device=dev).view(torch.uint8).view(n, 64)
    want = P.city64_batch(keys).cpu().numpy().view(np.uint64)
    assert (_u64(np.load(tmp_path / "digests.npy"))[:, 0] == want).all()
