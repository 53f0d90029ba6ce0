"""tests/world_ref.py proved on the CPU before tests/test_gpu_world.py relies on it: the W-rank model on
hand-written rounds (who wins when two sources put one key, a later round's overwrite, an absent key, a
source without keys, an owner that receives nothing), and route_records / route_replies against the real
collectives (pdht_amd.dist.exchange_records / exchange_replies) in spawned gloo processes on localhost at
world sizes 1 and 3, byte for byte, owner by owner and source by source."""
import os
import queue
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

import world_ref as WR
from test_table_cpu import _free_port


# ------------------------------------------------------------- the model ---
L, E = 8, 4


def _keys_owned_by(oracle, W, per_owner, seed=0):
    """`per_owner` distinct 8-byte keys for every owner r of a W-rank world: {r: keys [per_owner, 8]}."""
    k = np.unique(np.random.default_rng(seed).integers(0, 256, (64 * W * per_owner, L), dtype=np.uint8), axis=0)
    mb, _, rk = oracle.pdht_hash_fixed(k, 3, W)
    assert (mb % np.uint64(W) == rk).all() and len(np.unique(mb)) == len(k)
    out = {r: k[rk == r][:per_owner] for r in range(W)}
    assert all(len(v) == per_owner for v in out.values())
    return out


def _vals(*rows):
    return np.array(rows, np.uint8).reshape(len(rows), E)


def test_two_sources_put_one_key_the_higher_rank_wins(oracle):
    W = 3
    own = _keys_owned_by(oracle, W, 2)
    a, b = own[1][0], own[1][1]
    w = WR.World(W, [64] * W, oracle)
    st = w.put_round({2: (np.stack([a]), _vals([2] * E)),
                      0: (np.stack([a, b]), _vals([9] * E, [7] * E))})  # given out of rank order on purpose
    assert st[0].tolist() == [1, 0] and st[2].tolist() == [0]  # rank 2's record arrives after rank 0's
    got = w.get_round({1: np.stack([a, b])}, E, sentinel=0xC3)[1]
    assert got[1].tolist() == [0, 0] and (got[0] == _vals([2] * E, [7] * E)).all()
    inb = w.route_put({0: (np.stack([a, b]), _vals([9] * E, [7] * E)), 2: (np.stack([a]), _vals([2] * E))})
    assert inb[1].src.tolist() == [0, 0, 2] and inb[1].pos.tolist() == [0, 1, 0]
    assert len(inb[0].src) == len(inb[2].src) == 0 and inb[0].rows.shape == (0, 16)


def test_twice_in_one_batch_and_overwritten_in_a_later_round(oracle):
    W = 2
    own = _keys_owned_by(oracle, W, 2)
    a, b = own[0][0], own[1][0]
    w = WR.World(W, {0: 64, 1: 64}, oracle)
    st = w.put_round({1: (np.stack([a, b, a]), _vals([1] * E, [2] * E, [3] * E))})
    assert st[1].tolist() == [1, 0, 0]  # the last record of an mbits wins
    v, s = w.get_round({0: np.stack([a, b, a])}, E)[0]  # a query repeats a key
    assert s.tolist() == [0, 0, 0] and (v == _vals([3] * E, [2] * E, [3] * E)).all()
    st = w.put_round({0: (np.stack([a]), _vals([4] * E))})  # round 2: another source overwrites
    assert st[0].tolist() == [0]
    v, s = w.get_round({1: np.stack([a, b])}, E)[1]
    assert s.tolist() == [0, 0] and (v == _vals([4] * E, [2] * E)).all()
    assert [len(m.d) for m in w.models] == [1, 1] and [m.batches for m in w.models] == [2, 1]


def test_absent_key_empty_source_and_idle_owner(oracle):
    W = 3
    own = _keys_owned_by(oracle, W, 3)
    a, b, never = own[0][0], own[0][1], own[0][2]
    w = WR.World(W, lambda r: 64, oracle)
    none = (np.zeros((0, L), np.uint8), np.zeros((0, E), np.uint8))
    st = w.put_round({0: none, 2: (np.stack([a, b]), _vals([5] * E, [6] * E))})
    assert st[0].shape == (0,) and st[2].tolist() == [0, 0]
    assert [len(m.d) for m in w.models] == [2, 0, 0]  # owners 1 and 2 received nothing
    assert [m.batches for m in w.models] == [1, 0, 0]
    got = w.get_round({0: np.zeros((0, L), np.uint8), 1: np.stack([never, a, own[1][0]])}, E, sentinel=0xC3)
    assert got[0][0].shape == (0, E) and got[0][1].shape == (0,)
    assert got[1][1].tolist() == [2, 0, 2]  # NotFound at an owner that holds keys and at one that holds none
    assert (got[1][0] == _vals([0xC3] * E, [5] * E, [0xC3] * E)).all()  # not OK: the sentinel stays


def test_collision_and_a_full_owner(oracle):
    W = 2
    own = _keys_owned_by(oracle, W, 70)
    w = WR.World(W, [64, 64], oracle)
    k = own[1][:3]
    inb = w.route_put({0: (k, _vals([1] * E, [2] * E, [3] * E))})
    inb[1].rows[1, 0] ^= 0x40  # another key under the same mbits
    st, by_owner = w.apply_put(inb, {0: 3})
    assert st[0].tolist() == [0, 0, 0] and by_owner[1].tolist() == [0, 0, 0]
    v, s = w.get_round({1: k}, E, sentinel=0xC3)[1]
    assert s.tolist() == [0, 3, 0] and (v == _vals([1] * E, [0xC3] * E, [3] * E)).all()
    # 70 distinct keys at an owner of 64 slots: 3 are present, 61 fit, the sequential order drops the last 6
    vals = np.zeros((70, E), np.uint8)
    st = w.put_round({1: (own[1], vals)})[1]
    assert (st[:64] == 0).all() and (st[64:] == 2).all() and w.models[1].dropped == 6
    # ... unless the caller names the losers (what a device's schedule decided)
    w2 = WR.World(W, [64, 64], oracle)
    inb = w2.route_put({1: (own[1], vals)})
    lost = {int(x) for x in inb[1].mbits[:6]}
    st = w2.apply_put(inb, {1: 70}, dropped={1: lost})[0][1]
    assert (st[:6] == 2).all() and (st[6:] == 0).all() and w2.models[1].dropped == 6
    assert w2.get_round({0: own[1][:7]}, E)[0][1].tolist() == [2] * 6 + [0]


# ------------------------------------------------------------ the routing ---
RB, REPLY = 48, 24
N_OF = {1: [300], 3: [500, 0, 137]}  # records per rank; one rank of the 3-rank world sends nothing


def _records(rank, world):
    """Rank `rank`'s forged records in bucket order and its offsets.  Owner 1 of the 3-rank world gets no
    record from rank 2, and every byte of a record depends on (rank, position)."""
    n = N_OF[world][rank]
    rng = np.random.default_rng(77 + rank)
    mb = rng.integers(1, 1 << 62, n).astype(np.uint64)
    if world == 3 and rank == 2:
        mb[mb % np.uint64(3) == 1] += np.uint64(1)
    order, offs = WR.bucket_order((mb % np.uint64(world)).astype(np.int64), world)
    rec = rng.integers(0, 256, (n, RB), dtype=np.uint8)
    rec[:, 4:8] = np.frombuffer(np.uint32(rank).tobytes(), np.uint8)
    rec[:, 12:16] = order.astype(np.uint32).view(np.uint8).reshape(-1, 4)
    rec[:, 16:24] = mb[order].view(np.uint8).reshape(-1, 8)
    return rec, offs


def _replies(rank, mine):
    """The owner's answer to each record where it stands: {owner, arrival position, source rank, source
    index, mbits}."""
    rep = np.zeros((mine.shape[0], REPLY), np.uint8)
    rep[:, 0:2] = np.frombuffer(np.uint16(rank).tobytes(), np.uint8)
    rep[:, 2:4] = np.arange(mine.shape[0], dtype=np.uint16).view(np.uint8).reshape(-1, 2)
    rep[:, 4:8] = mine[:, 4:8]
    rep[:, 8:16] = mine[:, 16:24]
    rep[:, 16:20] = mine[:, 12:16]
    return rep


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pdht_amd import dist as D
        rec, offs = _records(rank, world)
        offs_t = torch.from_numpy(offs)
        mine, counts = D.exchange_records(torch.from_numpy(rec), offs_t)
        rep = _replies(rank, mine.numpy())
        back = D.exchange_replies(torch.from_numpy(rep), offs_t, counts)
        q.put({"rank": rank, "mine": mine.numpy(), "counts": counts.numpy(), "back": back.numpy()})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("as_torch", [False, True])
@pytest.mark.parametrize("WORLD", [1, 3])
def test_stand_ins_route_as_the_collectives_do(WORLD, as_torch, collectives):
    res = collectives[WORLD]
    wrap = torch.from_numpy if as_torch else (lambda a: a)
    sent = {r: _records(r, WORLD) for r in range(WORLD)}
    inbound, counts = WR.route_records({r: wrap(sent[r][0]) for r in sent}, {r: wrap(sent[r][1]) for r in sent},
                                       WORLD)
    assert len(inbound) == len(counts) == WORLD
    for r in range(WORLD):  # owner by owner
        assert type(inbound[r]) is type(wrap(sent[0][0]))
        assert np.asarray(inbound[r]).shape == res[r]["mine"].shape
        assert (np.asarray(inbound[r]) == res[r]["mine"]).all()
        assert (counts[r] == res[r]["counts"]).all()
    replies = [wrap(_replies(r, res[r]["mine"])) for r in range(WORLD)]
    back = WR.route_replies(replies, {r: sent[r][1] for r in sent}, counts)
    for s in range(WORLD):  # source by source
        assert np.asarray(back[s]).shape == res[s]["back"].shape == (N_OF[WORLD][s], REPLY)
        assert (np.asarray(back[s]) == res[s]["back"]).all()
        # and what came back is what the docstrings promise: reply p answers the sender's record p
        rec, offs = sent[s]
        b = res[s]["back"]
        assert (b[:, 0:2].copy().view(np.uint16).ravel() == np.repeat(np.arange(WORLD), np.diff(offs))).all()
        assert (b[:, 4:8].copy().view(np.uint32).ravel() == s).all()
        assert (b[:, 8:16] == rec[:, 16:24]).all() and (b[:, 16:20] == rec[:, 12:16]).all()
    if WORLD == 3:
        assert res[1]["counts"].tolist()[1:] == [0, 0] and res[0]["counts"][1] == 0  # the idle sender and pair
        # arrival order: source 0's records, then source 2's, each in its bucket order
        for r in range(WORLD):
            src = res[r]["mine"][:, 4:8].copy().view(np.uint32).ravel()
            assert (np.diff(src.astype(np.int64)) >= 0).all()


def test_a_subset_of_the_ranks_sends(collectives):
    """Ranks that are not named send nothing: the 3-rank world with its silent rank 1 left out."""
    sent = {r: _records(r, 3) for r in (0, 2)}
    inbound, counts = WR.route_records({r: sent[r][0] for r in sent}, {r: sent[r][1] for r in sent}, 3)
    for r in range(3):
        assert (inbound[r] == collectives[3][r]["mine"]).all() and (counts[r] == collectives[3][r]["counts"]).all()
    back = WR.route_replies([_replies(r, inbound[r]) for r in range(3)], {r: sent[r][1] for r in sent}, counts)
    assert sorted(back) == [0, 2]
    for s in back:
        assert (back[s] == collectives[3][s]["back"]).all()


@pytest.fixture(scope="module")
def collectives():
    """{world: [what every rank's exchange_records and exchange_replies returned]}, run once."""
    out = {}
    ctx = mp.get_context("spawn")
    for world in sorted(N_OF):
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res, deadline = [], time.monotonic() + 240
        while len(res) < world:
            try:
                res.append(q.get(timeout=0.5))
            except queue.Empty:  # a rank that died leaves the others waiting in the collective: end them all
                if any(p.exitcode not in (None, 0) for p in procs) or time.monotonic() > deadline:
                    for p in procs:
                        p.kill()
                    pytest.fail(f"world {world}: exit codes {[p.exitcode for p in procs]}")
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        out[world] = sorted(res, key=lambda x: x["rank"])
    return out
