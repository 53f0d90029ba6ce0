"""The Meraculous traversal's step (bench/Meraculous/UU_traversal_final.h:252, :444) as a W-rank world on
one device, W DeviceTables, against the dict world of tests/world_ref.py and the sequential models of
tests/table_rmw_ref.py:
  round 0  every rank puts its keys, the value's word 0 = UNUSED
  claim    bucket_records(get) -> route_records -> DeviceTable.cswap at word_offset = key slot ->
           route_replies -> scatter_rows by the records' index at +12
  update   bucket_put_records -> route_records -> DeviceTable.update_records -> route_replies -> scatter_rows
  get      bucket_records(get) -> route_records -> DeviceTable.get -> route_replies -> get_resolve
route_records / route_replies stand in for the two collectives (proved against them under gloo in
tests/test_world_ref_cpu.py).  What only the flow shows: for every key exactly one claimant in the whole
world sees UNUSED, and it is the first in the owner's arrival order -- lowest source rank, then position."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_rmw_ref as R  # noqa: E402
import world_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

GET, HT = 0, 3
L, E = 16, 16  # value = {used flag, payload}
SLOT = WR.slot_of(L)
B = WR.rowbytes_of(L, E)
UNUSED, USED = 0x00000000FFFFFFFF, 0x7000000000000001
PER = 150  # keys a rank puts


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle
    oracle.lib()
    return oracle


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def values_of(flag, payload):
    return np.stack([np.full(len(payload), flag, np.uint64), np.asarray(payload, np.uint64)], axis=1).view(np.uint8)


def back_in_callers_order(replies_by_owner, rec, offs, counts, width, n_of, dev, fill=0xEE):
    """route_replies, then scatter_rows by the index every record carries at +12."""
    back = WR.route_replies(replies_by_owner, offs, counts)
    got = {}
    for s in sorted(rec):
        out = torch.full((n_of[s], width), fill, dtype=torch.uint8, device=dev)
        P.scatter_rows(back[s], P.record_fields(rec[s], L)[3], out=out)
        got[s] = out.cpu().numpy()
    return got


@pytest.mark.parametrize("W", [1, 3, 8])
def test_claim_update_get_world(dev, oracle, W):
    rng = np.random.default_rng(1000 + W)
    pool = np.unique(rng.integers(0, 256, (W * PER + 80, L), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))]
    assert len(pool) >= W * PER + 2
    mine = {s: pool[s * PER:(s + 1) * PER] for s in range(W)}
    ghost, ghost2 = pool[W * PER], pool[W * PER + 1]  # keys nobody puts
    world = WR.World(W, lambda r: 1024, oracle)
    tabs = [P.DeviceTable(1024, B, dev) for _ in range(W)]

    # ---- round 0: every rank puts its keys, flag UNUSED ----
    batches = {s: (mine[s], values_of(UNUSED, np.arange(PER) + 1000 * s)) for s in range(W)}
    rec, offs = {}, {}
    for s in range(W):
        rec[s], offs[s] = P.bucket_put_records(up(batches[s][0], dev), up(batches[s][1], dev), W, src_rank=s,
                                               ht_index=HT)
    inbound, counts = WR.route_records(rec, offs, W)
    for r in range(W):
        tabs[r].put_records(inbound[r], status=False)
    want = world.put_round(batches)
    assert all((want[s] == 0).all() for s in range(W))  # distinct keys: all stored
    nbatch = [m.batches for m in world.models]

    # ---- claim round: own keys and the next rank's, one key twice, one key nobody put ----
    claims = {}
    for s in range(W):
        c = np.concatenate([mine[s], mine[(s + 1) % W], mine[s][5:6], ghost[None]])
        claims[s] = c[rng.permutation(len(c))]
    rec, offs = {}, {}
    for s in range(W):
        rec[s], offs[s] = P.bucket_records(up(claims[s], dev), W, msg_type=GET, src_rank=s, ht_index=HT)
    inbound, counts = WR.route_records(rec, offs, W)
    want_in = world.route_keys(claims)
    replies, want_rep = [], {s: np.full((len(claims[s]), 16), 0xEE, np.uint8) for s in range(W)}
    for r in range(W):
        replies.append(tabs[r].cswap(inbound[r], SLOT, UNUSED, USED))  # the records where they stand
        state = R.state_of(world.models[r])
        wr = R.cswap_ref(state, want_in[r].mbits, SLOT, UNUSED, USED)  # in arrival order
        R.into_model(world.models[r], state)
        nbatch[r] += 1 if len(want_in[r].mbits) else 0
        assert (replies[r].cpu().numpy() == wr).all()
        for s in range(W):
            of_s = want_in[r].src == s
            want_rep[s][want_in[r].pos[of_s]] = wr[of_s]
    got = back_in_callers_order(replies, rec, offs, counts, 16, {s: len(claims[s]) for s in range(W)}, dev)
    saw_unused = {}  # key -> [(source, position)] of the claimants that saw UNUSED
    claimants = {}
    for s in range(W):
        assert (got[s] == want_rep[s]).all(), f"source {s}"
        old = np.ascontiguousarray(got[s][:, 8:16]).view(np.uint64).ravel()
        for i, k in enumerate(map(bytes, claims[s])):
            claimants.setdefault(k, []).append((s, i))
            if k == bytes(ghost):
                assert got[s][i, 0] == 0 and old[i] == 0
                continue
            assert got[s][i, 0] == 1 and old[i] in (UNUSED, USED)
            if old[i] == UNUSED:
                saw_unused.setdefault(k, []).append((s, i))
    put_keys = {bytes(k) for s in range(W) for k in mine[s]}
    assert set(saw_unused) == put_keys
    for k in put_keys:  # exactly one winner: lowest source rank, then position
        assert len(claimants[k]) >= 2 and len({s for s, _ in claimants[k]}) >= min(W, 2)
        assert saw_unused[k] == [min(claimants[k])]
    assert max(len(v) for v in claimants.values()) >= 3 or W == 1  # the key claimed twice by one rank

    # ---- update round: the winners write a new value (flag USED), everybody also a key nobody holds ----
    batches = {}
    for s in range(W):
        won = np.array([np.frombuffer(k, np.uint8) for k, v in sorted(saw_unused.items()) if v[0][0] == s],
                       np.uint8).reshape(-1, L)
        keys = np.concatenate([won, ghost[None], ghost2[None], ghost[None]])
        vals = values_of(USED, 5000 * (s + 1) + np.arange(len(keys)))
        order = rng.permutation(len(keys))
        batches[s] = (keys[order], vals[order])
    rec, offs = {}, {}
    for s in range(W):
        rec[s], offs[s] = P.bucket_put_records(up(batches[s][0], dev), up(batches[s][1], dev), W, src_rank=s,
                                               ht_index=HT)
    inbound, counts = WR.route_records(rec, offs, W)
    want_in = world.route_put(batches)
    status, want_st = [], {s: np.full(len(batches[s][0]), 0xEE, np.uint8) for s in range(W)}
    for r in range(W):
        status.append(tabs[r].update_records(inbound[r]))
        state = R.state_of(world.models[r])
        ws = R.update_ref(state, want_in[r].mbits, want_in[r].rows)
        R.into_model(world.models[r], state)
        nbatch[r] += 1 if len(want_in[r].mbits) else 0
        assert (status[r].cpu().numpy() == ws).all()
        for s in range(W):
            of_s = want_in[r].src == s
            want_st[s][want_in[r].pos[of_s]] = ws[of_s]
    got = back_in_callers_order([x.view(-1, 1) for x in status], rec, offs, counts, 1,
                                {s: len(batches[s][0]) for s in range(W)}, dev)
    for s in range(W):
        assert (got[s][:, 0] == want_st[s]).all(), f"source {s}"
        is_ghost = np.array([bytes(k) in (bytes(ghost), bytes(ghost2)) for k in batches[s][0]])
        assert (got[s][is_ghost, 0] == 3).all() and (got[s][~is_ghost, 0] == 0).all()
    for r in range(W):
        assert tabs[r].counts()[:3] == (len(world.models[r].d), 0, nbatch[r])
    assert sum(len(m.d) for m in world.models) == W * PER  # nothing was inserted

    # ---- get round: every rank reads every key back, and the two nobody holds ----
    queries = {s: np.concatenate([pool[:W * PER], ghost[None], ghost2[None]])[rng.permutation(W * PER + 2)]
               for s in range(W)}
    want = world.get_round(queries, E, 0, 0xC3)
    kd, rec, offs = {}, {}, {}
    for s in range(W):
        kd[s] = up(queries[s], dev)
        rec[s], offs[s] = P.bucket_records(kd[s], W, msg_type=GET, src_rank=s, ht_index=HT)
    inbound, counts = WR.route_records(rec, offs, W)
    replies = [tabs[r].get(inbound[r], head=8) for r in range(W)]
    back = WR.route_replies(replies, offs, counts)
    winner_payload = {}
    for s in range(W):
        for k, v in zip(map(bytes, batches[s][0]), batches[s][1]):
            winner_payload[k] = v
    for s in range(W):
        vals = torch.full((len(queries[s]), E), 0xC3, dtype=torch.uint8, device=dev)
        v, st = P.get_resolve(back[s], kd[s], E, head=8, index=P.record_fields(rec[s], L)[3], values=vals)
        v, st = v.cpu().numpy(), st.cpu().numpy()
        assert (st == want[s][1]).all() and (v == want[s][0]).all(), f"source {s}"
        for i, k in enumerate(map(bytes, queries[s])):
            if k in put_keys:
                assert st[i] == 0 and (v[i] == winner_payload[k]).all()  # the winner's value, flag USED
            else:
                assert st[i] == 2
