"""A W-rank put/get world in plain Python and numpy: libmpipdht's client (putget.c:50-100) and server
(init.c:173-290) restated for the tests of the whole flow
  put  bucket_put_records -> dist.exchange_records -> DeviceTable.put_records
  get  bucket_records(get) -> exchange_records -> DeviceTable.get -> dist.exchange_replies -> get_resolve.
Every owner's table is the dict model of tests/test_gpu_table.py (Model); nothing here restates it.  The
digests come from the oracle (oracle.pdht_hash_fixed), owner = mbits % W.  route_records / route_replies
are the one-process stand-ins of the two collectives, by slicing and concatenating numpy arrays or torch
tensors; tests/test_world_ref_cpu.py proves them byte for byte against the collectives under gloo before
tests/test_gpu_world.py uses them in place of a multi-GPU run.  Nothing here touches a GPU."""
from dataclasses import dataclass

import numpy as np

from test_gpu_table import Model

OK, NOT_FOUND, COLLISION = 0, 2, 3          # pdht.h:199-204, what get_resolve writes
STORED, SUPERSEDED, DROPPED = 0, 1, 2       # DeviceTable.put_records' status


def slot_of(L, key_slot=0):
    return key_slot if key_slot else (L + 7) // 8 * 8


def rowbytes_of(L, E, key_slot=0):
    """A put record's row (what the table stores): the key slot and the value padded to 8."""
    return slot_of(L, key_slot) + (E + 7) // 8 * 8


def bucket_order(owner, W):
    """(order, offsets) of a stable bucketing by owner: bucket r = order[offsets[r]:offsets[r+1]], the
    caller's positions in the caller's order."""
    owner = np.asarray(owner, np.int64)
    order = np.argsort(owner, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=W))]).astype(np.int64)
    return order, offs


@dataclass
class Inbound:
    """An owner's inbound put batch in arrival order: the source rank and the position in that source's
    batch of every record, its mbits and its row (rows may be edited before apply_put)."""
    src: np.ndarray
    pos: np.ndarray
    mbits: np.ndarray
    rows: np.ndarray


def _as_list(x, W):
    return [x(r) for r in range(W)] if callable(x) else [x[r] for r in range(W)]


class World:
    """W owners, each a Model of `capacity_of_rank[r]` (a list, a dict or a function of r) entries."""

    def __init__(self, W, capacity_of_rank, oracle=None):
        if oracle is None:
            from oracle import oracle
            oracle.lib()
        self.W, self.oracle = W, oracle
        self.models = [Model(c) for c in _as_list(capacity_of_rank, W)]

    def place(self, keys):
        """(mbits uint64 [n], owner int64 [n]) of keys [n, L]."""
        keys = np.ascontiguousarray(keys, np.uint8)
        if len(keys) == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.int64)
        mb, _, rk = self.oracle.pdht_hash_fixed(keys, 3, self.W)
        owner = (mb % np.uint64(self.W)).astype(np.int64)
        assert (owner == rk).all()
        return mb, owner

    # ------------------------------------------------------------------ put ---
    def route_put(self, batches, key_slot=0):
        """batches {src: (keys [n, L], values [n, E])} -> [Inbound per owner]: the records of source 0 that
        the owner owns in source 0's key order, then source 1's, ... (exchange_records' order); sources
        that did not put contribute nothing."""
        rows = {}
        for s, (keys, values) in batches.items():
            keys, values = np.asarray(keys, np.uint8), np.asarray(values, np.uint8)
            n, L = keys.shape
            E = values.shape[1]
            assert values.shape[0] == n
            slot, self.rowbytes = slot_of(L, key_slot), rowbytes_of(L, E, key_slot)
            rows[s] = np.zeros((n, self.rowbytes), np.uint8)
            rows[s][:, :L] = keys
            rows[s][:, slot:slot + E] = values
        return self.route_keys({s: b[0] for s, b in batches.items()}, rows)

    def route_keys(self, keys_by_src, rows_by_src=None):
        """[Inbound per owner] of {src: keys [n, L]} (rows: the keys themselves unless given), in
        exchange_records' order."""
        assert keys_by_src, "a round needs at least one source (it may hold no keys)"
        per = [[] for _ in range(self.W)]
        for s in sorted(keys_by_src):
            assert 0 <= s < self.W
            keys = np.asarray(keys_by_src[s], np.uint8)
            rows = keys if rows_by_src is None else rows_by_src[s]
            mb, owner = self.place(keys)
            order, offs = bucket_order(owner, self.W)
            for r in range(self.W):
                pos = order[offs[r]:offs[r + 1]]
                per[r].append((np.full(len(pos), s, np.int64), pos, mb[pos], rows[pos]))
        return [Inbound(*(np.concatenate([g[i] for g in groups]) for i in range(4))) for groups in per]

    def apply_put(self, inbound, sizes, dropped=None):
        """Every owner applies its inbound batch one record after the other (init.c:223-241: find by mbits,
        insert if absent, overwrite).  sizes {src: n}.  Returns (status per source in the caller's key
        order {src: uint8 [n]}, status per owner in arrival order [uint8 [m]]): 0 stored and final,
        1 superseded by a later record of the same inbound batch, 2 dropped.
        dropped {owner: mbits the owner found no slot for}: which NEW mbits lose when a batch overflows is
        the device's schedule, so a test reads that set from the device; their records get 2 and the rest
        is applied in order.  Without it the sequential order decides (the later new mbits lose)."""
        by_src = {s: np.full(n, 0xEE, np.uint8) for s, n in sizes.items()}
        by_owner = []
        for r, (inb, model) in enumerate(zip(inbound, self.models)):
            lost = np.zeros(len(inb.mbits), bool)
            if dropped and len(dropped.get(r, ())):
                lost = np.isin(inb.mbits, np.array(sorted(dropped[r]), np.uint64))
            keep = ~lost
            st = np.full(len(inb.mbits), DROPPED, np.uint8)
            held = {k for k in model.d if k != 0} | {int(k) for k in inb.mbits[keep] if k != 0}
            batches = model.batches + (1 if len(inb.mbits) else 0)
            if len(held) <= model.capacity:
                st[keep] = model.put_fast(inb.mbits[keep], inb.rows[keep])  # cannot overflow
            else:
                st[keep] = model.put(inb.mbits[keep], inb.rows[keep])
            model.dropped += int(lost.sum())
            model.batches = batches  # a batch counts even when every record of it was dropped
            by_owner.append(st)
            for s in by_src:
                of_s = inb.src == s
                by_src[s][inb.pos[of_s]] = st[of_s]
        assert all((v != 0xEE).all() for v in by_src.values())  # every record arrived at exactly one owner
        return by_src, by_owner

    def put_round(self, batches, key_slot=0):
        """One put round; the status every record gets, per source in the caller's key order."""
        inbound = self.route_put(batches, key_slot)
        return self.apply_put(inbound, {s: len(b[0]) for s, b in batches.items()})[0]

    # ------------------------------------------------------------------ get ---
    def get_round(self, queries, E, key_slot=0, sentinel=0):
        """queries {src: keys [n, L]} -> {src: (values uint8 [n, E], status uint8 [n])} in the caller's
        order (putget.c:50-59): the owner finds by mbits alone (init.c:192-220); 2 NotFound when it holds
        nothing, 3 Collision when the entry's key is another one, else 0 OK and the value.  Rows that are
        not OK keep `sentinel`."""
        out = {}
        for s, keys in queries.items():
            keys = np.asarray(keys, np.uint8)
            n, L = keys.shape
            slot = slot_of(L, key_slot)
            values = np.full((n, E), sentinel, np.uint8)
            status = np.full(n, NOT_FOUND, np.uint8)
            mb, owner = self.place(keys)
            for i in range(n):
                e = self.models[owner[i]].d.get(int(mb[i]))
                if e is None:
                    continue
                row = e[1]
                if (row[:L] != keys[i]).any():
                    status[i] = COLLISION
                else:
                    status[i] = OK
                    values[i] = row[slot:slot + E]
            out[s] = (values, status)
        return out

    def replies(self, r, mbits, head):
        """Owner r's replies to requests for `mbits` where they stand (DeviceTable.get's bytes)."""
        return self.models[r].replies(np.asarray(mbits, np.uint64), head, self.rowbytes)


# ------------------------------------------------ the collectives' stand-ins ---
def _ints(t):
    return [int(x) for x in t.tolist()]


def _cat(parts):
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    import torch
    return torch.cat(parts)


def route_records(records_by_src, offsets_by_src, W):
    """dist.exchange_records on one process.  records_by_src {src rank: records [n, stride]} in bucket
    order, offsets_by_src {src rank: offsets [W + 1]}; ranks that are not named send nothing.  Returns
    (inbound [W]: every record owner r receives, grouped by source rank in rank order, each group in its
    source's bucket order; recv_counts [W]: int64 [W] per owner, the records it received from each rank)."""
    assert records_by_src and set(records_by_src) == set(offsets_by_src)
    srcs = sorted(records_by_src)
    offs = {s: _ints(offsets_by_src[s]) for s in srcs}
    for s in srcs:
        assert 0 <= s < W and len(offs[s]) == W + 1 and offs[s][0] == 0 and offs[s][W] == len(records_by_src[s])
    inbound, counts = [], []
    for r in range(W):
        inbound.append(_cat([records_by_src[s][offs[s][r]:offs[s][r + 1]] for s in srcs]))
        c = np.zeros(W, np.int64)
        for s in srcs:
            c[s] = offs[s][r + 1] - offs[s][r]
        counts.append(c)
    return inbound, counts


def route_replies(replies_by_owner, offsets_by_src, counts):
    """dist.exchange_replies on one process.  replies_by_owner [W]: one row per record route_records
    delivered to that owner, in that order; offsets_by_src and counts as given to / returned by
    route_records.  Returns {src rank: replies [n, reply bytes]} in that source's bucket order: reply p
    answers its record p."""
    W = len(replies_by_owner)
    assert len(counts) == W
    start = [np.concatenate([[0], np.cumsum(np.asarray(c, np.int64))]) for c in counts]
    for r in range(W):
        assert len(replies_by_owner[r]) == start[r][W], f"owner {r}: {len(replies_by_owner[r])} replies " \
                                                        f"for {start[r][W]} records received"
    back = {}
    for s in sorted(offsets_by_src):
        offs = _ints(offsets_by_src[s])
        parts = []
        for r in range(W):
            assert int(counts[r][s]) == offs[r + 1] - offs[r]  # what owner r sends is what s awaits from it
            parts.append(replies_by_owner[r][int(start[r][s]):int(start[r][s + 1])])
        back[s] = _cat(parts)
    return back
