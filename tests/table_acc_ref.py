"""The sequential model of the table's accumulate (include/pdht_hip_table_acc.h) for the tests: a plain
loop over the dict state {mbits: row} of tests/table_rmw_ref.py, one record after the other in position
order, as a pdht_acc (libpdht/pdht.h:349) would act on the owner's table if the reference performed it.
Nothing here knows of winner words, waves or atomics, imports the library or touches a GPU.

Integers are numpy integers of the type's width, so they wrap as the device's do.  For doubles the model
keeps, per word it touched, every addend in position order (the word's old value first): `seq` is their
position-order sum, `exact` their math.fsum, `abs` the sum of their magnitudes and `n` their number --
what the any-order bound gamma_n * sum|x_i| of the header is made of."""
import math

import numpy as np

ADDED, DROPPED, NOT_FOUND = 0, 2, 3  # DeviceTable.acc_records' status

U = 2.0 ** -53


def gamma(n):
    return n * U / (1 - n * U)


def acc_ref(state, mbits, rows, dtype, value_offset, elems, insert, dropped=(), capacity=None):
    """Applies the batch to `state` in place.  dtype: np.int32, np.int64 or np.float64.  Returns
    (status uint8 [m], sums): sums is {} for integers, and for doubles {(mbits, k): dict(seq=, exact=, abs=,
    n=)} for every word (entry, element k) the batch added into; the state holds `seq`.
    insert: an absent mbits is created with the whole row of its first record, later ones add.
    dropped: the set of mbits the device reported as dropped (overflow only: which new mbits lose is the
    device's schedule); their records get status 2 and nothing else happens to them.  capacity: when
    given, the model asserts that what it inserts fits (mbits 0 has a slot of its own)."""
    dt = np.dtype(dtype)
    assert dt in (np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.float64))
    lo, hi = value_offset, value_offset + elems * dt.itemsize
    dropped = {int(k) for k in dropped}
    m = len(mbits)
    status = np.zeros(m, np.uint8)
    addends = {}
    work = np.uint32 if dt.itemsize == 4 and dt.kind == "i" else np.uint64 if dt.kind == "i" else np.float64
    for p, k in enumerate(np.asarray(mbits, np.uint64).tolist()):
        row = state.get(k)
        if row is None:
            if not insert:
                status[p] = NOT_FOUND
                continue
            if k in dropped:
                status[p] = DROPPED
                continue
            state[k] = np.array(rows[p], np.uint8)  # the whole row of the first record: key slot and value
            if dt.kind == "f":
                for j, x in enumerate(state[k][lo:hi].view(np.float64).tolist()):
                    addends[(k, j)] = [x]
            continue
        assert k not in dropped, "a present mbits is never dropped"
        region = row[lo:hi].view(work)  # a view: writing it writes the row
        add = np.ascontiguousarray(rows[p][lo:hi]).view(work)
        if dt.kind == "f":
            for j in range(elems):
                addends.setdefault((k, j), [float(region[j])]).append(float(add[j]))
            region += add  # IEEE double, position order
        else:
            region += add  # unsigned: wraps modulo 2^32 / 2^64, the two's complement sum
    if capacity is not None:
        assert sum(1 for k in state if k != 0) <= capacity
    sums = {}
    for key, xs in addends.items():
        seq = xs[0]
        for x in xs[1:]:
            seq += x
        sums[key] = dict(seq=seq, exact=math.fsum(xs), abs=math.fsum(abs(x) for x in xs), n=len(xs))
    return status, sums
