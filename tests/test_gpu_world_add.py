"""Create-if-absent (bench/Meraculous' table build, bench/diff's "create node if nobody has") as a world of
W = 1, 3 and 8 ranks on one device, W DeviceTables:
  create  bucket_put_records -> route_records -> DeviceTable.add_records(replies=True) at each owner
          -> route_replies -> get_resolve
route_records / route_replies stand in for the two collectives (proved against them under gloo in
tests/test_world_ref_cpu.py).  The ranks' key sets overlap and every value carries its source rank and
position, so whose create won shows: for every key exactly one record in the world is answered 0, the
first in its owner's arrival order, and every rank resolves that record's value from the replies of the
same trip -- no second exchange, no Collision."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import world_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

HT = 2
L, E = 13, 8  # 13-byte keys, one int64 value: source rank * 2^32 + position
SLOT = WR.slot_of(L)
B = WR.rowbytes_of(L, E)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def create_round(tabs, keys, values, W, dev):
    """One create round.  Returns per owner (records in arrival order, status) as numpy, and per source
    (values, resolve status, add status) in the caller's key order."""
    rec, offs, kd = {}, {}, {}
    for s in range(W):
        kd[s] = up(keys[s], dev)
        rec[s], offs[s] = P.bucket_put_records(kd[s], up(values[s].view(np.uint8).reshape(-1, E), dev), W,
                                               src_rank=s, ht_index=HT)
        assert rec[s].shape[1] == 24 + B
    inbound, counts = WR.route_records(rec, offs, W)
    owners, replies, status = [], [], []
    for r in range(W):
        st, rep = tabs[r].add_records(inbound[r], replies=True)
        if len(st):
            assert P.last_kernel() == "k_table_add_claim+k_table_add_write<8>+k_table_add_reply<16>"  # 4 words
        assert int((st == 2).sum()) == 0 and len(st) == int(counts[r].sum())
        owners.append((inbound[r].cpu().numpy(), st.cpu().numpy()))
        replies.append(rep)
        status.append(st.view(-1, 1))
    back, back_st = WR.route_replies(replies, offs, counts), WR.route_replies(status, offs, counts)
    sources = {}
    for s in range(W):
        index = P.record_fields(rec[s], L)[3]
        v, st = P.get_resolve(back[s], kd[s], E, head=8, index=index)
        mine = np.full(len(keys[s]), 9, np.uint8)
        mine[index.cpu().numpy()] = back_st[s].cpu().numpy().ravel()
        sources[s] = (v.cpu().numpy().view(np.int64).ravel(), st.cpu().numpy(), mine)
    return owners, sources


@pytest.mark.parametrize("W", [1, 3, 8])
def test_create_if_absent_world(dev, W):
    rng = np.random.default_rng(5000 + W)
    pool = np.unique(rng.integers(0, 4, (340, L), dtype=np.uint8) + 65, axis=0)[:300]
    assert len(pool) >= 250
    keys, values = {}, {}
    for s in range(W):  # overlapping sets, repeats inside a rank too
        idx = np.concatenate([rng.integers(0, len(pool), 400), rng.integers(0, 25, 150)])
        keys[s] = pool[idx[rng.permutation(len(idx))]]
        values[s] = (np.int64(s) << 32) + np.arange(len(idx), dtype=np.int64)
    tabs = [P.DeviceTable(1024, B, dev) for _ in range(W)]

    owners, sources = create_round(tabs, keys, values, W, dev)
    winner = {}  # key -> the value of the first record of it in its owner's arrival order
    for r, (rec, st) in enumerate(owners):
        seen = set()
        for p in range(len(rec)):
            k = bytes(rec[p, 24:24 + L])
            v = int(rec[p, 24 + SLOT:24 + SLOT + E].view(np.int64)[0])
            assert v >> 32 == int(rec[p, 4:8].view(np.int32)[0])  # the row carries its source rank
            if k in seen:
                assert st[p] == 4
            else:
                assert st[p] == 0 and k not in winner  # one owner per key, one creator per key
                seen.add(k)
                winner[k] = v
        assert tabs[r].counts()[:3] == (len(seen), 0, 1 if len(rec) else 0)
    everyone = {bytes(k) for s in range(W) for k in keys[s]}
    assert set(winner) == everyone
    zeros = 0
    for s in range(W):
        v, st, mine = sources[s]
        for i, k in enumerate(map(bytes, keys[s])):
            assert st[i] == WR.OK and v[i] == winner[k]  # every rank resolves the same winning value
            assert mine[i] == (0 if v[i] == values[s][i] else 4)
        zeros += int((mine == 0).sum())
    assert zeros == len(everyone)  # exactly one record in the world per key

    # a second round finds everything present
    before = [(t.counts(), [x.cpu().numpy() for x in t.entries()]) for t in tabs]
    owners, sources = create_round(tabs, keys, {s: values[s] + 1000000 for s in range(W)}, W, dev)
    for r in range(W):
        rec, st = owners[r]
        assert (st == 4).all()
        c0, c1 = before[r][0], tabs[r].counts()
        assert c1[:2] == c0[:2] and c1[2] == c0[2] + (1 if len(rec) else 0) and c1[3] - c0[3] >= len(rec)
        for a, b in zip(before[r][1], [x.cpu().numpy() for x in tabs[r].entries()]):
            assert a.tobytes() == b.tobytes()
    for s in range(W):
        v, st, mine = sources[s]
        assert (st == WR.OK).all() and (mine == 4).all()
        assert v.tolist() == [winner[k] for k in map(bytes, keys[s])]

    # another key with the mbits of a stored one: the owner answers 4 with the row it holds, and the client's
    # resolve sees another key's bytes there
    r = max(range(W), key=lambda x: len(owners[x][0]))
    forged = owners[r][0][:3].copy()
    forged[:, 24:24 + L] = 90
    st, rep = tabs[r].add_records(up(forged.view(np.int64), dev).view(torch.uint8).view(3, -1), replies=True)
    assert st.cpu().tolist() == [4, 4, 4]
    v, rst = P.get_resolve(rep, up(np.full((3, L), 90, np.uint8), dev), E, head=8)
    assert rst.cpu().tolist() == [WR.COLLISION] * 3
