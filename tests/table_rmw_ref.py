"""The sequential models of the table's update and compare-and-swap (include/pdht_hip_table_rmw.h) for
the tests: plain loops over a dict {mbits: row}, one record after the other in position order, as
pdht_update (libpdht/putget.c:278) and pdht_atomic_cswap (libpdht/atomics.c:81-154) act on the owner's
table.  Nothing here knows which record of an mbits "wins": that the device's two-kernel form equals
these loops is what the GPU tests show.  Nothing here imports the library or touches a GPU.

state: {int mbits: uint8 row [B]}; both functions change it in place.  A Model of tests/test_gpu_table.py
keeps {mbits: (-1, row)}: state_of / into_model convert."""
import numpy as np

STORED, SUPERSEDED, NOT_FOUND = 0, 1, 3  # DeviceTable.update_records' status


def update_ref(state, mbits, rows):
    """status uint8 [m] of an update batch: find by mbits; if present overwrite the row, else nothing."""
    m = len(mbits)
    status = np.zeros(m, np.uint8)
    writer = {}  # mbits -> the position whose row the entry holds, for this batch
    for p in range(m):
        k = int(mbits[p])
        if k not in state:
            status[p] = NOT_FOUND
            continue
        if k in writer:
            status[writer[k]] = SUPERSEDED  # its row is gone as of now
        state[k] = np.array(rows[p], np.uint8)
        writer[k] = p
    return status


def cswap_ref(state, mbits, word_offset, compare, desired):
    """replies uint8 [m, 16] of a compare-and-swap batch: {found, 7 zero bytes, old}; old = word, and
    word = desired when word == compare."""
    compare, desired = int(compare) & (2 ** 64 - 1), int(desired) & (2 ** 64 - 1)
    m = len(mbits)
    found, old = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    for p, k in enumerate(np.asarray(mbits, np.uint64).tolist()):
        row = state.get(k)
        if row is None:
            continue
        word = row[word_offset:word_offset + 8].view(np.uint64)  # a view: writing it writes the row
        found[p], old[p] = 1, word[0]
        if int(word[0]) == compare:
            word[0] = desired
    return np.stack([found, old], axis=1).view(np.uint8).reshape(m, 16)


def state_of(model):
    """The state of a Model (tests/test_gpu_table.py), rows copied."""
    return {k: np.array(v[1], np.uint8) for k, v in model.d.items()}


def into_model(model, state):
    model.d = {k: (-1, np.array(v, np.uint8)) for k, v in state.items()}
