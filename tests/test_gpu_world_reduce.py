"""Keep-the-best and flag sets (bench/Meraculous' extension flags, a relaxed distance, a smallest label) as a
world of W = 1, 3 and 8 ranks on one device, W DeviceTables, against dict models over all ranks' records:
  propose  bucket_put_records -> route_records -> DeviceTable.reduce_records(op, insert=True, replies=True)
           at each owner -> route_replies -> get_resolve
route_records / route_replies stand in for the two collectives (proved against them under gloo in
tests/test_world_ref_cpu.py).  Every source proposes a value per key; keys are shared between sources and
repeated within a batch.  After ONE trip every source holds the global result for each of its keys -- the
replies are the entries after the owner's whole inbound batch --, the key slot is the first record's and
intact (get_resolve reports no Collision)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import world_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

HT = 2
L, E = 13, 8  # 13-byte keys, one int64 value
SLOT = WR.slot_of(L)
B = WR.rowbytes_of(L, E)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def reduce_round(tabs, keys, values, op, W, dev):
    """One round.  Returns per source the resolved values (int64, the caller's key order) after the trip."""
    rec, offs, kd = {}, {}, {}
    for s in range(W):
        kd[s] = up(keys[s], dev)
        rec[s], offs[s] = P.bucket_put_records(kd[s], up(values[s].view(np.uint8).reshape(-1, E), dev), W,
                                               src_rank=s, ht_index=HT)
        assert rec[s].shape[1] == 24 + B
    inbound, counts = WR.route_records(rec, offs, W)
    replies = []
    for r in range(W):
        st, rep = tabs[r].reduce_records(inbound[r], torch.int64, op, SLOT, insert=True, replies=True)
        if len(st):
            assert P.last_kernel() == f"k_table_acc_claim+k_table_acc<i64,{op},insert>+k_table_add_reply<16>"  # 4 words
        assert int(st.count_nonzero()) == 0 and len(st) == int(counts[r].sum())
        replies.append(rep)
    back = WR.route_replies(replies, offs, counts)
    out = {}
    for s in range(W):
        v, st = P.get_resolve(back[s], kd[s], E, head=8, index=P.record_fields(rec[s], L)[3])
        assert (st.cpu().numpy() == WR.OK).all()  # found, and no Collision: the key slot is intact
        out[s] = v.cpu().numpy().view(np.int64).ravel()
    return out


@pytest.mark.parametrize("W", [1, 3, 8])
def test_global_minimum_and_flag_sets_in_one_trip(dev, W):
    rng = np.random.default_rng(6000 + W)
    pool = np.unique(rng.integers(0, 4, (340, L), dtype=np.uint8) + 65, axis=0)[:300]
    assert len(pool) >= 250
    keys, values, best = {}, {}, {}
    for s in range(W):  # overlapping sets, repeats inside a rank too
        idx = np.concatenate([rng.integers(0, len(pool), 400), rng.integers(0, 25, 150)])
        keys[s] = pool[idx[rng.permutation(len(idx))]]
        values[s] = rng.integers(-(1 << 40), 1 << 40, len(idx)).astype(np.int64)  # both signs: a signed minimum
        for k, v in zip(map(bytes, keys[s]), values[s].tolist()):
            best[k] = min(best.get(k, v), v)
    tabs = [P.DeviceTable(1024, B, dev) for _ in range(W)]

    got = reduce_round(tabs, keys, values, "min", W, dev)
    for s in range(W):
        assert got[s].tolist() == [best[k] for k in map(bytes, keys[s])]
    assert sum(t.counts()[0] for t in tabs) == len(best)
    assert any(v < 0 for v in best.values()) and any(v > 0 for v in best.values())

    # a second round with larger values changes nothing
    before = [[x.cpu().numpy() for x in t.entries()] for t in tabs]
    got = reduce_round(tabs, keys, {s: values[s] + (1 << 41) for s in range(W)}, "min", W, dev)
    for s in range(W):
        assert got[s].tolist() == [best[k] for k in map(bytes, keys[s])]
    for r in range(W):
        for a, b in zip(before[r], [x.cpu().numpy() for x in tabs[r].entries()]):
            assert a.tobytes() == b.tobytes()

    # flags: every source ORs bits into its keys' entries; against a dict of sets
    flag_tabs = [P.DeviceTable(1024, B, dev) for _ in range(W)]
    flags, sets = {}, {}
    for s in range(W):
        bit = rng.integers(0, 63, len(keys[s]))
        flags[s] = (np.int64(1) << bit).astype(np.int64)
        for k, b in zip(map(bytes, keys[s]), bit.tolist()):
            sets.setdefault(k, set()).add(b)
    got = reduce_round(flag_tabs, keys, flags, "or", W, dev)
    for s in range(W):
        assert got[s].tolist() == [sum(1 << b for b in sets[k]) for k in map(bytes, keys[s])]
