"""A numpy model of the table export (include/pdht_hip_table_iter.h) for the tests: it reads a COPY of a
table's storage by the documented layout --
    +0            u64 counters[4]
    +64           u64 tags[C + 1]     0 = empty, else the mbits stored there (tags[C]: 1 = mbits 0 present)
    +64+8(C+1)    u64 win[C + 1]
    +64+16(C+1)   rows[C + 1][B]
-- and returns what an export of a slot range must write.  Nothing here imports the library."""
import numpy as np

TILE = 1024  # kExportTile (pdht_amd/csrc/table_iter.h): the slots of a tile, counted from first_slot


def layout(capacity, rowbytes):
    """Byte offsets of (tags, winner words, rows) and the size of the storage."""
    tags = 64
    win = tags + 8 * (capacity + 1)
    rows = win + 8 * (capacity + 1)
    return tags, win, rows, rows + (capacity + 1) * rowbytes


def split(storage, capacity, rowbytes):
    """(tags u64 [C + 1], rows u8 [C + 1, B]) as views of a uint8 storage array."""
    storage = np.asarray(storage, np.uint8)
    t, w, r, end = layout(capacity, rowbytes)
    assert storage.size >= end
    return storage[t:w].view(np.uint64), storage[r:end].reshape(capacity + 1, rowbytes)


def forge_storage(capacity, rowbytes, live_slots, seed=0):
    """A storage image whose live slots are `live_slots`: a distinct non-zero tag in each ordinary one, 1 in
    the private one, noise in every row (a dead slot's row must never be exported) and in the winner words."""
    rng = np.random.default_rng(seed)
    t, w, r, end = layout(capacity, rowbytes)
    st = rng.integers(0, 256, end, dtype=np.uint8)
    st[:t] = 0
    tags = st[t:w].view(np.uint64)
    tags[:] = 0
    live = np.asarray(sorted(set(int(s) for s in live_slots)), np.int64)
    assert len(live) == 0 or (live[0] >= 0 and live[-1] <= capacity)
    tags[live] = (live.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) | np.uint64(1)
    if len(live) and live[-1] == capacity:
        tags[capacity] = 1
    st[:8] = np.frombuffer(np.uint64(len(live)).tobytes(), np.uint8)  # counters[0]
    return st


def export_ref(storage, capacity, rowbytes, first_slot=0, nslots=None, max_entries=None):
    """(mbits u64 [w], rows u8 [w, B], slots u32 [w], count2) of an export of [first_slot, first_slot + nslots):
    the live slots (tag != 0) in ascending order, the private slot reporting mbits 0; w = count2[1] =
    min(count2[0], max_entries)."""
    tags, rows = split(storage, capacity, rowbytes)
    if nslots is None:
        nslots = capacity + 1 - first_slot
    assert nslots >= 1 and 0 <= first_slot and first_slot + nslots <= capacity + 1
    slots = first_slot + np.flatnonzero(tags[first_slot:first_slot + nslots] != 0)
    n = len(slots)
    w = n if max_entries is None else min(n, int(max_entries))
    slots = slots[:w]
    mbits = tags[slots].copy()
    mbits[slots == capacity] = 0
    return mbits, rows[slots].copy(), slots.astype(np.uint32), (n, w)
