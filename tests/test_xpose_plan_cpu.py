"""Launch plan of the 64-B kernel (pdht_hip_xpose64_plan_for) and the tile
function the kernel indexes with (pdht_hip_xpose64_tiles): every tile of a
batch exactly once, no workgroup without a tile, for the round-blocked shape
at every R the tuning variants use and for the persistent shape.  No GPU."""
import numpy as np
import pytest

import pdht_amd as P

CUS = (1, 2, 8, 256, 304)
RS = (1, 2, 4, 8, 16)
DELTAS = (-65, -64, -1, 0, 1, 63, 64, 65)


def sizes(cus, R):
    G = 2 * 3 * cus * 4  # tiles of one round at 3 workgroups of 4 waves per CU
    ns = [0, 1, 63, 64, 65]
    for k in sorted({1, R, R + 1, 2 * R + 1}):
        ns += [k * G * 64 + d for d in DELTAS]
    return G, [n for n in ns if n >= 0]


def check_cover(plan, n):
    """Enumerate every (workgroup, round, d, wave) as the kernel does: a
    workgroup hashes its tiles below the batch's tile count."""
    ntiles = (n + 63) // 64
    if n == 0:
        assert plan.launches == 0
        return
    t = P.xpose64_tiles(plan)
    slots = plan.waves // 4
    assert t.shape == (plan.grid, plan.rounds_per_wg if plan.round_blocked else plan.rounds, 2, 4)
    # no workgroup without a tile: its smallest tile (first round, d 0, wave 0) is in the batch
    assert (t[:, 0, 0, 0] < ntiles).all()
    assert (t.reshape(plan.grid, -1).min(axis=1) == t[:, 0, 0, 0]).all()
    if plan.round_blocked:
        # a workgroup's tiles stay inside its round block (the kernel's `end`)
        q = np.arange(plan.grid, dtype=np.uint64) // np.uint64(slots)
        G = np.uint64(2 * plan.waves)
        lo = (q * np.uint64(plan.rounds_per_wg) * G)[:, None]
        flat = t.reshape(plan.grid, -1)
        assert (flat >= lo).all() and (flat < lo + np.uint64(plan.rounds_per_wg) * G).all()
    got = np.sort(t[t < ntiles])
    assert got.size == ntiles and (got == np.arange(ntiles, dtype=np.uint64)).all()


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("R", RS)
def test_round_blocked_covers_every_tile_once(cus, R):
    G, ns = sizes(cus, R)
    for n in ns:
        p = P.xpose64_plan(n, cus, R)
        ntiles = (n + 63) // 64
        rounds = -(-ntiles // G) if ntiles > G else (1 if n else 0)
        assert p.round_blocked == (1 if rounds > R else 0), (n, cus, R)
        if p.round_blocked:
            assert (p.waves, p.rounds, p.rounds_per_wg, p.launches) == (12 * cus, rounds, R, 1)
            assert (-(-rounds // R) - 1) * 3 * cus < p.grid <= -(-rounds // R) * 3 * cus
        check_cover(p, n)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("R", RS)
def test_up_to_R_rounds_the_plan_is_the_persistent_grid(cus, R):
    """With R >= rounds the round-blocked shape is the persistent launch."""
    G, ns = sizes(cus, R)
    for n in ns:
        ntiles = (n + 63) // 64
        if n == 0 or -(-ntiles // G) > R:
            continue
        p, q = P.xpose64_plan(n, cus, R), P.xpose64_plan(n, cus, 0)
        assert not p.round_blocked and not q.round_blocked
        assert [getattr(p, f) for f, _ in p._fields_] == [getattr(q, f) for f, _ in q._fields_]
        assert p.grid == min((n + 255) // 256, 3 * cus) and p.waves == 4 * p.grid and p.launches == 1
        check_cover(p, n)


@pytest.mark.parametrize("cus", CUS)
def test_persistent_and_histogram_plans(cus):
    G, ns = sizes(cus, 4)
    for n in ns:
        p = P.xpose64_plan(n, cus, 0)
        assert not p.round_blocked and p.rounds_per_wg == 0
        check_cover(p, n)
        h = P.xpose64_plan(n, cus, 2, hist=True)
        assert [getattr(h, f) for f, _ in h._fields_] == [getattr(p, f) for f, _ in p._fields_]
    # above 512 MiB of keys the persistent shape goes out in 8M-key launches
    p = P.xpose64_plan((20 << 20) + 5, cus, 0)
    assert (p.launches, p.grid, p.round_blocked) == (3, 3 * cus, 0)
    assert p.rounds == -(-(8 << 20) // 64 // (24 * cus))


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("R", RS)
def test_grid_fits_32_bits_at_8GiB(cus, R):
    n = (8 << 30) // 64
    p = P.xpose64_plan(n, cus, R)
    assert p.round_blocked and p.launches == 1 and 0 < p.grid < 2 ** 31
    # the first and the last workgroup's tiles
    ntiles = n // 64
    assert P.xpose64_tiles(p, 0, 1)[0, 0, 0, 0] == 0
    last = P.xpose64_tiles(p, p.grid - 1, 1)
    assert last[0, 0, 0, 0] < ntiles and ntiles - 1 in P.xpose64_tiles(p, p.grid - 3 * cus, 3 * cus)


def test_library_choice_and_bad_arguments():
    p = P.xpose64_plan(16 << 20, 256)  # the product's own shape for the flagship batch
    q = P.xpose64_plan(16 << 20, 256, p.rounds_per_wg)
    assert [getattr(p, f) for f, _ in p._fields_] == [getattr(q, f) for f, _ in q._fields_]
    assert p.launches == (1 if p.round_blocked else 2)
    check_cover(p, (16 << 20) // p.launches)  # (the first launch's tiles)
    with pytest.raises(P.PdhtError):
        P.xpose64_plan(64, 0)
    with pytest.raises(P.PdhtError):
        P.xpose64_tiles(p, p.grid, 1)
