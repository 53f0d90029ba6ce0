"""The sequential model of the table's insert-if-absent (include/pdht_hip_table_add.h) for the tests: a
plain loop over the dict state {mbits: row} of tests/table_rmw_ref.py, one record after the other in
position order, as the Portals put acts on the owner's match list (libpdht/poll.c:205-263: a put is
appended behind the entries that are there, and matching reaches the oldest).  Nothing here knows of
"first", "creator", winner words, waves or atomics, imports the library or touches a GPU."""
import numpy as np

CREATED, DROPPED, EXISTS = 0, 2, 4  # DeviceTable.add_records' status


def add_ref(state, mbits, rows, capacity=None, dropped=None):
    """Applies the batch to `state` in place: find by mbits; if absent, insert it with this record's row; if
    present, do nothing.  Returns (status uint8 [m], replies uint8 [m, 8 + B]): reply p is the head-8 get
    reply for mbits[p] on the state after the batch -- 1, seven zeros and the row, or all zeros when the
    mbits is not there.
    dropped: the set of mbits the device reported as dropped (overflow only: which new mbits lose is the
    device's schedule); their records get status 2 and nothing else happens to them.  The drop conditions
    are checked here: only new mbits are dropped (never mbits 0, which has a slot of its own), all records
    of an mbits share their fate (by construction: the set is of mbits), and with `capacity` given the
    entries stored are min(distinct new mbits, free slots) -- never short while free slots remain."""
    dropped = {int(k) for k in (dropped or ())}
    mb = np.asarray(mbits, np.uint64).tolist()
    m = len(mb)
    rows = np.asarray(rows, np.uint8)
    assert rows.ndim == 2 and len(rows) == m
    assert not (dropped & set(state)), "a present mbits is never dropped"
    assert 0 not in dropped, "mbits 0 has a slot of its own"
    assert dropped <= set(mb)
    if capacity is not None:
        free = capacity - sum(1 for k in state if k != 0)
        new = {k for k in mb if k not in state and k != 0}
        assert len(new) - len(dropped) == min(len(new), free), (len(new), len(dropped), free)
    status = np.zeros(m, np.uint8)
    for p, k in enumerate(mb):
        if k in state:
            status[p] = EXISTS
        elif k in dropped:
            status[p] = DROPPED
        else:
            state[k] = rows[p].copy()
            status[p] = CREATED
    # what a get of every record's mbits answers now
    replies = np.zeros((m, 8 + rows.shape[1]), np.uint8)
    held = {k: i for i, k in enumerate(state)}
    at = np.array([held.get(k, -1) for k in mb], np.int64)
    if m and held:
        table = np.stack(list(state.values()))
        replies[at >= 0, 0] = 1
        replies[at >= 0, 8:] = table[at[at >= 0]]
    return status, replies
