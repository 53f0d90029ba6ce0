"""Counting k-mers (bench/Meraculous, before the traversal claims them) as a W = 3 world on one device,
W DeviceTables, against a collections.Counter over all ranks' keys:
  count   bucket_put_records -> route_records -> DeviceTable.acc_records(insert=True) at each owner
  get     bucket_records(get) -> route_records -> DeviceTable.get -> route_replies -> get_resolve
route_records / route_replies stand in for the two collectives (proved against them under gloo in
tests/test_world_ref_cpu.py).  Every rank sends a count of 1 (or more) per occurrence; the owner creates
the entry from the first record it receives and adds the rest, so the key slot must be intact afterwards:
get_resolve compares it with the client's key and reports no Collision."""
import collections

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import world_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

GET, HT, W = 0, 2, 3
L, E = 13, 8  # 13-byte k-mers, one int64 count
SLOT = WR.slot_of(L)
B = WR.rowbytes_of(L, E)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_kmer_count_world(dev):
    from oracle import oracle
    oracle.lib()
    world = WR.World(W, lambda r: 256, oracle)  # placement only: owner = mbits % W
    rng = np.random.default_rng(3000)
    kmers = np.unique(rng.integers(0, 4, (320, L), dtype=np.uint8) + 65, axis=0)[:300]  # "ACGT"-like bytes
    assert len(kmers) >= 250
    ghost = np.full((1, L), 90, np.uint8)  # a key nobody counts
    hot = rng.integers(0, len(kmers), 6)
    reads, weights, total = {}, {}, collections.Counter()
    for s in range(W):  # heavy repeats inside every rank and across them
        idx = np.concatenate([rng.integers(0, len(kmers), 500), np.repeat(hot, 60), rng.integers(0, 20, 200)])
        idx = idx[rng.permutation(len(idx))]
        reads[s] = kmers[idx]
        weights[s] = rng.integers(1, 4, len(idx)).astype(np.int64)  # an occurrence counts 1 .. 3
        for k, w in zip(map(bytes, reads[s]), weights[s].tolist()):
            total[k] += w
    tabs = [P.DeviceTable(256, B, dev) for _ in range(W)]

    for rnd in (1, 2):  # the second round finds every k-mer present and only adds
        rec, offs = {}, {}
        for s in range(W):
            rec[s], offs[s] = P.bucket_put_records(up(reads[s], dev), up(weights[s].view(np.uint8).reshape(-1, E), dev),
                                                   W, src_rank=s, ht_index=HT)
            assert rec[s].shape[1] == 24 + B
        inbound, counts = WR.route_records(rec, offs, W)
        owners = world.place(kmers)[1]
        for r in range(W):
            st = tabs[r].acc_records(inbound[r], torch.int64, SLOT, insert=True)
            assert P.last_kernel() == "k_table_acc_claim+k_table_acc<i64,insert>"
            assert int(st.count_nonzero()) == 0 and len(st) == int(counts[r].sum())
            mine = {bytes(k) for k in kmers[owners == r]} & set(total)
            assert tabs[r].counts()[:3] == (len(mine), 0, rnd)
        assert sum(t.counts()[0] for t in tabs) == len(total)

        queries = {s: np.concatenate([kmers, ghost])[rng.permutation(len(kmers) + 1)] for s in range(W)}
        kd, rec, offs = {}, {}, {}
        for s in range(W):
            kd[s] = up(queries[s], dev)
            rec[s], offs[s] = P.bucket_records(kd[s], W, msg_type=GET, src_rank=s, ht_index=HT)
        inbound, counts = WR.route_records(rec, offs, W)
        back = WR.route_replies([tabs[r].get(inbound[r], head=8) for r in range(W)], offs, counts)
        for s in range(W):
            v, st = P.get_resolve(back[s], kd[s], E, head=8, index=P.record_fields(rec[s], L)[3])
            v, st = v.cpu().numpy().view(np.int64).ravel(), st.cpu().numpy()
            for i, k in enumerate(map(bytes, queries[s])):
                if k in total:
                    assert st[i] == WR.OK, f"source {s} key {i}: status {st[i]}"  # no Collision: the key slot is intact
                    assert v[i] == rnd * total[k]
                else:
                    assert st[i] == WR.NOT_FOUND
