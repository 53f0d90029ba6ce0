"""The whole put / get flow of a W-rank world on one device, W DeviceTables, bit-exact against the dict
world of tests/world_ref.py:
  put  bucket_put_records -> route_records -> DeviceTable.put_records -> status bytes -> route_replies ->
       scatter_rows
  get  bucket_records(get) -> route_records -> DeviceTable.get -> route_replies -> get_resolve
route_records / route_replies stand in for dist.exchange_records / exchange_replies; that they move the same
bytes is proved under gloo in tests/test_world_ref_cpu.py.  What the flow holds between its stages and no
per-kernel test does: records arrive grouped by source rank in rank order, each group in its source's key
order; reply p answers the sender's record p; the last record of an mbits in arrival order wins.  The
tables see the mbits they see in service: CityHash64 digests with mbits % W == r."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import world_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

GET = 0      # msg_type pdhtGet
HT = 3       # ht_index carried in every header
SENT = 0xC3  # what values hold where no OK reply lands

WS = (1, 2, 3, 8, 61, 257)
LS = (8, 13, 32, 64)
ES = (1, 8, 12, 40, 256)
BIG = (65, 4097, 1000)
ROUNDS = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- the cases ---
def sources_of(W, S):
    """S source ranks of a W-rank world, rank 0 and rank W - 1 among them."""
    S = min(S, W)
    return [0] if S == 1 else sorted({round(i * (W - 1) / (S - 1)) for i in range(S)})


def _world_cases():
    """W x L thinned to one (E, key_slot, head, sizes) each: everything rotates with the sum of the two
    indices, so that every E, both key_slot forms and both heads occur, each head with both key_slot forms.
    sizes: the keys per source, rotated by one source every round; it always holds 0 and 1, and where a
    world has fewer than three ranks the one source meets them in different rounds.  W = 257 is the slow one
    and has the fewest sources; its sizes are (0, 1, 65, big) over three sources, so that its first put round
    and its second get round bring 66 records to 257 owners: about 199 owners receive nothing and 51 one
    record (257 (256/257)^66 and 66 (256/257)^65), the m == 0 and m == 1 paths."""
    cases = []
    for iW, W in enumerate(WS):
        for iL, L in enumerate(LS):
            i = iW + iL
            S = min(W, 3 if W == 257 else 5 if W == 61 else 4)
            n = max(S, 3)
            sizes = (0, 1) + tuple(BIG[(i + j) % 3] for j in range(n - 2))
            sizes = sizes[i % n:] + sizes[:i % n]
            if W == 257:
                sizes = (0, 1, 65, BIG[1 + i % 2])
            cases.append((W, L, ES[i % 5], 32 if L <= 32 and i % 2 else 0, 1 if (i // 2) % 2 else 8, S, sizes))
    return cases


WORLD_CASES = _world_cases()


def get_tag(B, head):
    """pdht_table.hip table_get on replies that DeviceTable.get allocates (16-byte aligned, packed)."""
    return "k_table_get_bytes" if head == 1 else "k_table_get<16>" if (B // 8 + 1) % 2 == 0 else "k_table_get<8>"


def p16(rowbytes, stride, ptr):
    """pdht_table.hip table_put: rows move in 16-byte pieces only when all three are multiples of 16."""
    return rowbytes % 16 == 0 and stride % 16 == 0 and (ptr + 24) % 16 == 0


def test_world_cases_cover_the_grid():
    assert len(WORLD_CASES) == len(WS) * len(LS)
    assert {(c[0], c[1]) for c in WORLD_CASES} == {(W, L) for W in WS for L in LS}
    assert {c[2] for c in WORLD_CASES} == set(ES)
    assert {c[3] for c in WORLD_CASES} == {0, 32} and all(c[1] <= 32 for c in WORLD_CASES if c[3])
    assert {(c[4], bool(c[3])) for c in WORLD_CASES} == {(8, False), (8, True), (1, False), (1, True)}
    for W in WS:  # every world meets both heads, and a key slot of 32
        assert {c[4] for c in WORLD_CASES if c[0] == W} == {1, 8}
        assert {c[3] for c in WORLD_CASES if c[0] == W} == {0, 32}
    for L in LS:
        assert len({c[2] for c in WORLD_CASES if c[1] == L}) >= 4
    for W, L, E, key_slot, head, S, sizes in WORLD_CASES:
        src = sources_of(W, S)
        assert 1 <= len(src) == min(S, W) <= 5 and src[0] == 0 and src[-1] == W - 1
        assert 0 in sizes and 1 in sizes and set(sizes) <= {0, 1} | set(BIG)
        assert len(sizes) == (4 if W == 257 else max(len(src), 3))
        assert len(src) == len(sizes) or W < 3 or W == 257  # else every round has its empty and one-key source
    assert {n for c in WORLD_CASES for n in c[6]} == {0, 1} | set(BIG)
    for W in WS:
        assert {n for c in WORLD_CASES if c[0] == W for n in c[6]} == {0, 1} | set(BIG)
    # the three get kernels and every row width class the table moves
    tags = {get_tag(WR.rowbytes_of(c[1], c[2], c[3]), c[4]) for c in WORLD_CASES}
    assert tags == {"k_table_get_bytes", "k_table_get<16>", "k_table_get<8>"}
    # a put record's row is its stride - 24, so stride and rowbytes are never both multiples of 16: through
    # this flow a put always moves 8-byte pieces, wherever the records stand
    for c in WORLD_CASES:
        B = WR.rowbytes_of(c[1], c[2], c[3])
        assert P.put_record_bytes(c[1], c[2], c[3]) == 24 + B
        assert not any(p16(B, 24 + B, ptr) for ptr in (0, 8))


def distinct_keys(rng, n, L):
    k = np.unique(rng.integers(0, 256, (n + 64, L), dtype=np.uint8), axis=0)
    assert len(k) >= n
    return k[rng.permutation(len(k))][:n]


def plan(W, L, E, S, sizes, seed, rounds=ROUNDS):
    """The rounds of a case: [(batches {src: (keys, values)}, queries {src: keys})].  Keys come from a pool
    smaller than the batches, so sources overlap within a round and across rounds, and explicitly:
      1. every source with keys puts the round's hot key (the one-key source puts nothing else): the arrival
         order decides;  2. a batch of two or more keys ends with its first key again;
      3. every larger batch but that of the source whose record of it stayed puts the previous round's hot
         key, every larger query batch asks for both hot keys and the one-key query for the previous one;
      4. queries draw from keys that are never put as well;  5. a query batch ends with its first key again.
    The hot keys are outside the pool the batches draw from, so only these rules place them in a put."""
    rng = np.random.default_rng(seed)
    src = sources_of(W, S)
    K = max(8, 3 * max(sizes) // 4)
    never = K // 4 + 8
    pool = distinct_keys(rng, K + rounds + never, L)
    hot = K + np.arange(rounds)
    out, stayed = [], None
    for t in range(rounds):
        batches, queries = {}, {}
        put_sizes = [sizes[(i + t) % len(sizes)] for i in range(len(src))]
        for i, s in enumerate(src):
            n = put_sizes[i]
            idx = rng.integers(0, K, n)
            if n >= 2:
                idx[n - 1] = idx[0]
                if t and s != stayed:
                    idx[n // 3] = hot[t - 1]
            if n:
                idx[n // 2] = hot[t]
            batches[s] = (pool[idx], rng.integers(0, 256, (n, E), dtype=np.uint8))
            # the query sizes run one source ahead of the put sizes where there are three (the one large
            # query batch then belongs to neither this round's nor the last round's large writer), else behind
            n = sizes[(i + t + (1 if len(sizes) == 3 else len(sizes) - 1)) % len(sizes)]
            idx = rng.integers(0, K + rounds + never, n)
            if n >= 2:
                idx[n - 1] = idx[0]
                idx[2], idx[3] = hot[max(t - 1, 0)], K + rounds
            if n:
                idx[n // 2] = hot[t] if n >= 2 or t == 0 else hot[t - 1]
            queries[s] = pool[idx]
        stayed = max((s for s, n in zip(src, put_sizes) if n), default=None)  # its record of hot[t] came last
        out.append((batches, queries))
    return out


def capacities(oracle, W, rounds_):
    """Per owner the smallest power of two >= max(64, 2 x the distinct mbits it ever holds)."""
    keys = np.concatenate([b[0] for batches, _ in rounds_ for b in batches.values()])
    mb, _, rk = oracle.pdht_hash_fixed(keys, 3, W)
    held = np.bincount(np.unique(np.stack([rk.astype(np.uint64), mb]), axis=1)[0].astype(np.int64), minlength=W)
    caps = [max(64, 1 << int(2 * h - 1).bit_length()) if h else 64 for h in held]
    assert all(c >= 2 * h and c & (c - 1) == 0 for c, h in zip(caps, held))
    return caps, held


# --------------------------------------------------------------- the flow ---
class Flow:
    """W tables on one device and the two rounds over them; every stage is compared with the model's."""

    def __init__(self, dev, W, L, E, key_slot, head, caps, stream=None):
        self.dev, self.W, self.L, self.E, self.key_slot, self.head, self.stream = dev, W, L, E, key_slot, head, stream
        self.B = WR.rowbytes_of(L, E, key_slot)
        self.tabs = [P.DeviceTable(c, self.B, dev) for c in caps]
        self.keep = []  # nothing the side stream may still read is freed before the test ends
        if stream is not None:
            torch.cuda.synchronize(dev)  # the tables were emptied on the default stream

    def on(self):
        """torch's own work (copies, slices, concatenations, read-backs) on the flow's stream."""
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def up(self, a):
        with self.on():
            t = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t

    def host(self, t):
        with self.on():
            return np.ascontiguousarray(t.cpu().numpy())

    def check_inbound(self, inbound, want, msg_type, fields):
        """Every owner's inbound records against the model's arrival order: the header carries the record's
        own source rank and position, the mbits is the key's digest and belongs to this owner."""
        with self.on():
            allin = torch.cat(inbound)
        self.keep.append(allin)
        ty, sr, hi, ix, mb = (self.host(f) for f in fields(allin)[:5])
        owner = np.repeat(np.arange(self.W), [len(x) for x in inbound])
        assert [len(x) for x in inbound] == [len(w.src) for w in want]
        mb = mb.view(np.uint64)
        assert (mb % np.uint64(self.W) == owner.astype(np.uint64)).all()
        assert (ty == msg_type).all() and (hi == HT).all()
        assert (sr == np.concatenate([w.src for w in want])).all()
        assert (ix.view(np.uint32) == np.concatenate([w.pos for w in want])).all()
        assert (mb == np.concatenate([w.mbits for w in want])).all()
        body = np.concatenate([w.rows for w in want])
        assert (self.host(allin)[:, 24:24 + body.shape[1]] == body).all()  # key (and value) with their pads
        assert (self.host(allin)[:, 24 + body.shape[1]:] == 0).all()

    def put(self, world, batches, edit=None, full_owner=None):
        """One put round.  edit(inbound tensors, model inbound): changes both before the owners apply them.
        full_owner: the owner whose batch overflows; what it dropped is read from its status."""
        W, L, E, ks, st = self.W, self.L, self.E, self.key_slot, self.stream
        rec, offs = {}, {}
        for s in sorted(batches):
            rec[s], offs[s] = P.bucket_put_records(self.up(batches[s][0]), self.up(batches[s][1]), W, key_slot=ks,
                                                   src_rank=s, ht_index=HT, stream=st)
            assert rec[s].shape[1] == 24 + self.B
        with self.on():
            inbound, counts = WR.route_records(rec, offs, W)
        want_in = world.route_put(batches, ks)
        self.check_inbound(inbound, want_in, P.PDHT_PUT, lambda t: P.put_record_fields(t, L, E, ks))
        if edit is not None:
            with self.on():
                edit(inbound, want_in)
        status = []
        for r in range(W):
            status.append(self.tabs[r].put_records(inbound[r], stream=st))
            assert P.last_kernel() == "k_table_claim+k_table_write<8>"
        self.keep += [rec, inbound, status]
        dropped = None
        if full_owner is not None:
            dropped = {full_owner: self.read_dropped(world, full_owner, want_in[full_owner],
                                                     self.host(status[full_owner]))}
        want_src, want_owner = world.apply_put(want_in, {s: len(b[0]) for s, b in batches.items()}, dropped)
        with self.on():
            allst = torch.cat(status)
        assert (self.host(allst) == np.concatenate(want_owner)).all()  # each owner's vector is the model's
        with self.on():
            back = WR.route_replies([x.view(-1, 1) for x in status], offs, counts)
        got = {}
        for s in sorted(batches):
            n = len(batches[s][0])
            with self.on():
                out = torch.full((n, 1), 0xEE, dtype=torch.uint8, device=self.dev)
            P.scatter_rows(back[s], P.put_record_fields(rec[s], L, E, ks)[3], out=out, stream=st)
            self.keep += [back[s], out]
            got[s] = self.host(out)[:, 0]
            assert (got[s] == want_src[s]).all(), f"source {s}"  # in the caller's key order
        cnt = [t.counts_dev(stream=st) for t in self.tabs]
        with self.on():
            cnt = torch.stack(cnt)
        cnt = self.host(cnt)
        assert (cnt[:, 0] == [len(m.d) for m in world.models]).all()
        assert (cnt[:, 1] == [m.dropped for m in world.models]).all()
        assert (cnt[:, 2] == [m.batches for m in world.models]).all()
        return got, want_in

    def read_dropped(self, world, r, inb, st):
        """test_gpu_table_edges.py::test_overflow_part_way's reading of an overflowing batch: which new mbits
        found no slot is the device's choice and the only thing taken from it; all records of one mbits
        share the fate, a present mbits is never dropped, and exactly the free slots are won."""
        model = world.models[r]
        lost = st == 2
        lost_keys, kept_keys = set(inb.mbits[lost].tolist()), set(inb.mbits[~lost].tolist())
        assert not (lost_keys & kept_keys)
        old = {k for k in model.d if k != 0}
        assert old & set(inb.mbits.tolist()) <= kept_keys and 0 not in lost_keys
        won = kept_keys - old - {0}
        assert lost_keys, "the batch was meant to overflow"
        assert len(won) == model.capacity - len(old)
        return lost_keys

    def get(self, world, queries):
        """One get round; returns {src: (values, status)} as read from the device (already compared)."""
        W, L, E, ks, st, head = self.W, self.L, self.E, self.key_slot, self.stream, self.head
        kd, rec, offs = {}, {}, {}
        for s in sorted(queries):
            kd[s] = self.up(queries[s])
            rec[s], offs[s] = P.bucket_records(kd[s], W, msg_type=GET, src_rank=s, ht_index=HT, stream=st)
        with self.on():
            inbound, counts = WR.route_records(rec, offs, W)
        want_in = world.route_keys(queries)
        self.check_inbound(inbound, want_in, GET, lambda t: P.record_fields(t, L))
        replies = []
        for r in range(W):
            replies.append(self.tabs[r].get(inbound[r], head=head, stream=st))  # the records where they stand
            assert tuple(replies[r].shape) == (len(want_in[r].mbits), head + self.B)
            if len(want_in[r].mbits):
                assert P.last_kernel() == get_tag(self.B, head)
        with self.on():
            allrep = torch.cat(replies)
            back = WR.route_replies(replies, offs, counts)
        self.keep += [rec, inbound, replies, allrep, back]
        assert (self.host(allrep) == np.concatenate([world.replies(r, want_in[r].mbits, head)
                                                     for r in range(W)])).all()
        want = world.get_round(queries, E, ks, SENT)
        got = {}
        for s in sorted(queries):
            n = len(queries[s])
            with self.on():
                vals = torch.full((n, E), SENT, dtype=torch.uint8, device=self.dev)
                stat = torch.full((n,), 0xEE, dtype=torch.uint8, device=self.dev)
            v, sv = P.get_resolve(back[s], kd[s], E, head=head, key_slot=ks, index=P.record_fields(rec[s], L)[3],
                                  values=vals, status=stat, stream=st)
            self.keep += [vals, stat]
            got[s] = (self.host(v), self.host(sv))
            assert (got[s][1] == want[s][1]).all(), f"source {s}"
            assert (got[s][0] == want[s][0]).all(), f"source {s}"  # rows that are not OK still hold SENT
        self.asked = want_in
        return got


def check_plan(world_log, S):
    """What the rounds were built to contain did happen (on the model)."""
    same_round = twice = overwritten = absent = repeated = False
    holder = {}  # key -> the source whose record of it the owner holds
    for t, (inbound, batches, queries, answers, winners) in enumerate(world_log):
        for inb in inbound:
            order = np.lexsort((inb.src, inb.mbits))
            mb, sr = inb.mbits[order], inb.src[order]
            eq = mb[1:] == mb[:-1]
            same_round |= bool((eq & (sr[1:] != sr[:-1])).any())
            twice |= bool((eq & (sr[1:] == sr[:-1])).any())
        absent |= any((a[1] == 2).any() for a in answers.values())
        repeated |= any(len(np.unique(q, axis=0)) < len(q) for q in queries.values())
        asked = {r: set(map(bytes, q)) for r, q in queries.items()}
        for k, s in winners.items():  # overwritten by another source than the one whose record was held
            if not overwritten and holder.get(k, s) != s:
                overwritten = S < 3 or any(k in a for r, a in asked.items() if r not in (s, holder[k]))
        holder.update(winners)
    assert twice and absent and repeated
    assert same_round or S < 2
    assert overwritten or S < 2


def last_writers(inbound, L):
    """{key bytes: source rank of the record that stays} of one round's inbound batches."""
    out = {}
    for inb in inbound:
        for p in range(len(inb.src)):
            out[inb.rows[p, :L].tobytes()] = int(inb.src[p])
    return out


@pytest.mark.parametrize("W,L,E,key_slot,head,S,sizes", WORLD_CASES)
def test_world_rounds(dev, oracle, W, L, E, key_slot, head, S, sizes):
    rounds_ = plan(W, L, E, S, sizes, seed=W * 1000 + L * 10 + E)
    caps, held = capacities(oracle, W, rounds_)
    dry = WR.World(W, caps, oracle)  # no put can overflow: shown on the model before the device is touched
    for batches, _ in rounds_:
        assert all((st != 2).all() for st in dry.put_round(batches, key_slot).values())
    assert all(m.dropped == 0 and 2 * len(m.d) <= c for m, c in zip(dry.models, caps))
    assert [len(m.d) for m in dry.models] == held.tolist()
    world, flow, log, per_owner = WR.World(W, caps, oracle), Flow(dev, W, L, E, key_slot, head, caps), [], []
    for batches, queries in rounds_:
        _, inbound = flow.put(world, batches)
        answers = flow.get(world, queries)
        log.append((inbound, batches, queries, answers, last_writers(inbound, L)))
        per_owner += [len(inb.src) for inb in inbound] + [len(inb.src) for inb in flow.asked]
    check_plan(log, len(sources_of(W, S)))
    if W == 257:  # half of what _world_cases expects of the two 66-record rounds
        per_owner = np.array(per_owner)
        assert (per_owner == 0).sum() >= 200 and (per_owner == 1).sum() >= 50


# ------------------------------------------------------------- collision ---
def test_collision_through_the_flow(dev, oracle):
    """One key byte of a few inbound records changes between the exchange and the owner (their mbits does
    not): the owner stores them under the mbits (init.c keys by mbits alone), and the client that asks for
    the original key reads Collision and keeps its sentinel; every other record is untouched."""
    W, L, E, key_slot, head, n = 3, 13, 12, 32, 8, 300
    rng = np.random.default_rng(5)
    keys = distinct_keys(rng, 3 * n, L)
    batches = {s: (keys[s * n:(s + 1) * n], rng.integers(0, 256, (n, E), dtype=np.uint8)) for s in range(3)}
    caps, _ = capacities(oracle, W, [(batches, None)])
    world, flow = WR.World(W, caps, oracle), Flow(dev, W, L, E, key_slot, head, caps)
    hit = {}

    def edit(inbound, want_in):
        for r in range(W):
            m = len(want_in[r].src)
            for p in (1, m // 2, m - 2):  # one record of each source's group; its neighbours stay as they are
                j = (p * 5) % L
                inbound[r][p, 24 + j] ^= 0x40
                want_in[r].rows[p, j] ^= 0x40
                hit[int(want_in[r].src[p]), int(want_in[r].pos[p])] = r

    st, _ = flow.put(world, batches, edit=edit)
    assert len(hit) == 9 and all((v == 0).all() for v in st.values())
    got = flow.get(world, {s: batches[(s + 1) % 3][0] for s in range(3)})  # another rank asks
    for s in range(3):
        want = np.zeros(n, np.uint8)
        want[[p for (src, p) in hit if src == (s + 1) % 3]] = 3
        assert (got[s][1] == want).all() and int((want == 3).sum()) == 3
        assert (got[s][0][want == 3] == SENT).all()
        assert (got[s][0][want == 0] == batches[(s + 1) % 3][1][want == 0]).all()  # every other record: its value


# ------------------------------------------------------ an owner fills up ---
def test_an_owner_fills_up(dev, oracle):
    """W = 3; owner 1 has 64 slots, holds 40 keys and is sent 60 new ones, each several times and from three
    sources, next to puts of the keys it holds.  Which of the new mbits it kept is read from its status
    (read_dropped); from there the model decides: the status every source gets back, that every client which
    later gets a dropped key reads NotFound, and that the two other owners lose nothing."""
    W, L, E, key_slot, head, full = 3, 8, 8, 0, 8, 1
    rng = np.random.default_rng(11)
    keys = distinct_keys(rng, 4000, L)
    mb, _, rk = oracle.pdht_hash_fixed(keys, 3, W)
    assert len(np.unique(mb)) == len(keys)
    mine, others = keys[rk == full], keys[rk != full]
    old, new, elsewhere = mine[:40], mine[40:100], others[:500]
    caps = [1024, 64, 1024]
    world, flow = WR.World(W, caps, oracle), Flow(dev, W, L, E, key_slot, head, caps)

    def batch(k):
        k = k[rng.permutation(len(k))]
        return k, rng.integers(0, 256, (len(k), E), dtype=np.uint8)

    st, _ = flow.put(world, {0: batch(np.concatenate([old[:25], elsewhere[:100]])), 2: batch(old[15:])})
    assert all((v != 2).all() for v in st.values()) and len(world.models[full].d) == 40
    second = {s: batch(np.concatenate([new, new[::2], old[s::3], elsewhere[100 * s:100 * s + 300]]))
              for s in range(3)}
    st, inbound = flow.put(world, second, full_owner=full)
    model = world.models[full]
    assert len(model.d) == 64 and model.dropped > 0
    lost = {k for s in range(3) for k, x in zip(map(bytes, second[s][0]), st[s]) if x == 2}
    assert len(lost) == 60 - 24 and lost <= set(map(bytes, new))  # 24 slots were free
    assert all((inbound[r].mbits % np.uint64(W) == r).all() for r in range(W))
    assert world.models[0].dropped == world.models[2].dropped == 0
    asked = {s: np.concatenate([new, old, elsewhere])[rng.permutation(600)] for s in range(3)}
    got = flow.get(world, asked)
    for s in range(3):
        is_lost = np.array([bytes(k) in lost for k in asked[s]])
        assert (got[s][1][is_lost] == 2).all() and (got[s][1][~is_lost] == 0).all()
        assert (got[s][0][is_lost] == SENT).all()
    # the same batch again: tags are final, the same mbits lose, the rest is overwritten
    st2, _ = flow.put(world, second, full_owner=full)
    assert all(((st2[s] == 2) == (st[s] == 2)).all() for s in range(3))
    flow.get(world, asked)


# ------------------------------------------- records read where they stand ---
@pytest.mark.parametrize("L,E,key_slot", [(8, 8, 0), (13, 12, 0), (13, 40, 32), (8, 1, 32)])
def test_records_read_where_they_stand(dev, oracle, L, E, key_slot):
    """With one source, an owner can apply rec[offs[r]:offs[r+1]] as a view of the sender's buffer.  Where
    the stride is 8 mod 16 and offs[r] is odd the view starts 8 mod 16, the address at which rows at +24 are
    16-byte aligned.  It must leave the same table and give the same status and replies as the concatenated
    copy, and the kernel tag must be what pdht_table.hip's p16 rule says for each placement: a put record's
    row is its stride - 24, so rowbytes and stride are never both multiples of 16 and every placement of
    such records (the view, the aligned copy, a copy at 8 mod 16) moves 8-byte pieces.  The 16-byte write
    needs records wider than their row: where rowbytes is a multiple of 16, a fourth placement copies them
    to a stride 8 bytes wider at 8 mod 16, and there the tag must name the 16-byte write."""
    W, n, head = 3, 4097, 8
    rng = np.random.default_rng(L * 100 + E)
    keys = distinct_keys(rng, 3000, L)[rng.integers(0, 3000, n)]
    while True:  # until a bucket starts at an odd record
        rk = oracle.pdht_hash_fixed(keys[:n], 3, W)[2]
        if (rk == 0).sum() % 2 or (rk <= 1).sum() % 2:
            break
        n -= 1
    assert n > 4090
    keys = keys[:n]
    values = rng.integers(0, 256, (n, E), dtype=np.uint8)
    caps, _ = capacities(oracle, W, [({0: (keys, values)}, None)])
    B = WR.rowbytes_of(L, E, key_slot)
    kd, vd = (torch.from_numpy(a).to(dev) for a in (keys, values))
    rec, offs = P.bucket_put_records(kd, vd, W, key_slot=key_slot, src_rank=0, ht_index=HT)
    copies, counts = WR.route_records({0: rec}, {0: offs}, W)
    o = [int(x) for x in offs.tolist()]
    stride = rec.shape[1]
    assert stride == 24 + B and rec.data_ptr() % 16 == 0
    starts, tags = set(), set()
    world = WR.World(W, caps, oracle)
    want_in = world.route_put({0: (keys, values)}, key_slot)
    want_st = world.apply_put(want_in, {0: n})[1]

    def at_8_mod_16(view, wide):
        """A copy of the records that starts 8 mod 16, its stride `wide` bytes."""
        m = len(view)
        buf = torch.zeros(m * wide // 8 + 2, dtype=torch.int64, device=dev).view(torch.uint8)
        out = buf[8:8 + m * wide].view(m, wide)
        out[:, :stride].copy_(view)
        assert out.data_ptr() % 16 == 8
        return out[:, :stride] if wide == stride else out

    for r in range(W):
        view = rec[o[r]:o[r + 1]]
        assert view.data_ptr() == rec.data_ptr() + o[r] * stride and copies[r].data_ptr() % 16 == 0
        starts.add(view.data_ptr() % 16)
        placed = [view, copies[r], at_8_mod_16(view, stride)]
        if B % 16 == 0:  # records wider than their row: the one form whose rows can move 16 bytes at a time
            placed.append(at_8_mod_16(view, stride + 8))
        out = []
        for records in placed:
            tab = P.DeviceTable(caps[r], B, dev)
            st = tab.put_records(records)
            piece = 16 if p16(B, records.stride(0), records.data_ptr()) else 8
            assert P.last_kernel() == f"k_table_claim+k_table_write<{piece}>"
            tags.add(piece)
            rep = tab.get(records, head=head)  # the requests read in place too
            out.append((st.cpu().numpy(), rep.cpu().numpy(), tab.counts()[:3]))
        assert (out[0][0] == want_st[r]).all()
        assert (out[0][1] == world.replies(r, want_in[r].mbits, head)).all()
        for other in out[1:]:
            assert (other[0] == out[0][0]).all() and (other[1] == out[0][1]).all() and other[2] == out[0][2]
    assert o[1] % 2 == 1 or o[2] % 2 == 1
    assert starts == ({0, 8} if stride % 16 == 8 else {0})  # a view did start 8 mod 16
    assert tags == ({8, 16} if B % 16 == 0 else {8})


# ------------------------------------------------------------ side stream ---
def test_rounds_on_a_side_stream(dev, oracle):
    """The whole put and get round with stream= passed to every call, torch's own copies and concatenations
    on the same stream and nothing on the default stream: the same answers as on the default stream."""
    W, L, E, key_slot, head, S, sizes = 8, 13, 40, 32, 1, 4, (1000, 0, 1, 4097)
    rounds_ = plan(W, L, E, S, sizes, seed=99, rounds=2)
    caps, _ = capacities(oracle, W, rounds_)
    results = []
    for stream in (None, torch.cuda.Stream(device=dev)):
        world, flow = WR.World(W, caps, oracle), Flow(dev, W, L, E, key_slot, head, caps, stream=stream)
        got = []
        for batches, queries in rounds_:
            got.append((flow.put(world, batches)[0], flow.get(world, queries)))
        torch.cuda.synchronize(dev)
        results.append(got)
    for (st0, g0), (st1, g1) in zip(*results):
        for s in st0:
            assert (st0[s] == st1[s]).all()
            assert (g0[s][0] == g1[s][0]).all() and (g0[s][1] == g1[s][1]).all()
