"""Plain numpy / Python references of the device-resident table (include/pdht_hip_table.h)
for the tests: where linear probing puts an mbits and what a put costs in inspected slots, and a
vectorised last-writer-wins table for batches of millions of records.  Nothing here imports the library;
tests/test_table_ref_cpu.py proves these against each other and against the dict model of
tests/test_gpu_table.py before the GPU tests rely on them."""
import numpy as np

MIX = 0x9E3779B97F4A7C15  # 2^64 / golden ratio
M64 = (1 << 64) - 1


def log2_capacity(capacity):
    k = int(capacity).bit_length() - 1
    assert capacity == 1 << k and 64 <= capacity <= 1 << 31
    return k


def home_high(mb, capacity):
    """The table's home: the high log2(C) bits of the multiplicative mix."""
    return ((int(mb) * MIX) & M64) >> (64 - log2_capacity(capacity))


def home_low(mb, capacity):
    """The wrong home (the low bits of the mbits), to show what the tests would catch."""
    return int(mb) & (capacity - 1)


def probe_walk(mbits_in_insert_order, capacity, home=home_high):
    """Sequential linear probing, slot by slot as the kernel walks: (slot of each mbits, 1 + displacement of
    each).  mbits 0 takes no ordinary slot (its slot is `capacity`) and costs 1.  Quadratic when the homes
    pile up; probe_model computes the same without the walk."""
    tags = [0] * capacity
    slots, cost = [], []
    for mb in mbits_in_insert_order:
        mb = int(mb)
        if mb == 0:
            slots.append(capacity)
            cost.append(1)
            continue
        h, n = home(mb, capacity), 1
        while tags[h] != 0 and tags[h] != mb:
            h, n = (h + 1) & (capacity - 1), n + 1
            assert n <= capacity, "more distinct mbits than slots"
        tags[h] = mb
        slots.append(h)
        cost.append(n)
    return np.array(slots, np.int64), np.array(cost, np.int64)


def probe_model(mbits_in_insert_order, capacity, home=home_high):
    """probe_walk's result in Python integers, with the walk over occupied slots replaced by a
    next-free-slot forest (path-halving union-find over the ring of slots), so that piled-up homes cost no
    more than spread ones.  Returns (slot of each mbits, 1 + displacement of each): the slots a put of an
    mbits that is PRESENT inspects, and the slots its first put inspected when nobody raced it.  A repeated
    mbits gets the slot and cost of its first occurrence."""
    nxt = list(range(capacity))  # nxt[s] == s: s is free; else a slot further along the ring
    where = {}
    used = 0
    slots, cost = [], []
    for mb in mbits_in_insert_order:
        mb = int(mb)
        if mb == 0:
            slots.append(capacity)
            cost.append(1)
            continue
        h = home(mb, capacity)
        s = where.get(mb)
        if s is None:
            assert used < capacity, "more distinct mbits than slots"
            s = h
            while nxt[s] != s:
                nxt[s] = nxt[nxt[s]]
                s = nxt[s]
            nxt[s] = (s + 1) & (capacity - 1)
            where[mb] = s
            used += 1
        slots.append(s)
        cost.append(1 + ((s - h) & (capacity - 1)))
    return np.array(slots, np.int64), np.array(cost, np.int64)


def clusters(slots, capacity):
    """The cluster (maximal run of occupied slots on the ring) of each given ordinary slot, as a label per
    entry of `slots` (mbits 0's private slot `capacity` gets -1), and the number of clusters.  Which keys
    sit in a cluster, and the sum of their displacements, do not depend on the insertion order; where
    inside it each key sits does."""
    slots = np.asarray(slots, np.int64)
    occ = np.zeros(capacity, bool)
    occ[slots[slots < capacity]] = True
    if occ.all():
        lab = np.zeros(capacity, np.int64)
        n = 1
    else:
        starts = occ & ~np.roll(occ, 1)  # an occupied slot behind a free one
        lab = np.cumsum(starts) - 1
        n = int(starts.sum())
        lab[lab < 0] = n - 1  # the run that wraps past slot 0 belongs to the last start
        lab[~occ] = -1
    out = np.full(len(slots), -1, np.int64)
    out[slots < capacity] = lab[slots[slots < capacity]]
    return out, n


# ------------------------------------------------------- last writer wins, vectorised ---
def put_ref(mbits, rows, state=None):
    """One put batch that cannot overflow, applied to `state` (None: an empty table): returns (status,
    state).  status[p] is 0 where record p is the last of its mbits in the batch, 1 elsewhere.  The state
    is (keys, rows) with the keys sorted ascending and the rows in the same order."""
    mbits = np.asarray(mbits, np.uint64)
    m = len(mbits)
    status = np.ones(m, np.uint8)
    if state is None:
        state = (np.zeros(0, np.uint64), np.zeros((0, rows.shape[1]), np.uint8))
    if m == 0:
        return status, state
    keys, first_rev = np.unique(mbits[::-1], return_index=True)  # sorted keys, their last position
    last = m - 1 - first_rev
    status[last] = 0
    old_k, old_r = state
    keep = ~np.isin(old_k, keys)  # entries this batch does not overwrite
    k = np.concatenate([old_k[keep], keys])
    r = np.concatenate([old_r[keep], rows[last]])
    order = np.argsort(k, kind="stable")
    return status, (k[order], r[order])


def replies_ref(state, mbits, head, B):
    """The replies of a get (head + B bytes each) from put_ref's state: byte 0 = found, then zeros up to
    `head`, then the row; all zeros when the mbits is absent."""
    keys, rows = state
    q = np.asarray(mbits, np.uint64)
    out = np.zeros((len(q), head + B), np.uint8)
    if len(keys) == 0 or len(q) == 0:
        return out
    at = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    found = keys[at] == q
    out[found, 0] = 1
    out[found, head:] = rows[at[found]]
    return out
