"""The sequential model of the table's reduce (include/pdht_hip_table_reduce.h) for the tests: a plain loop
over the dict state {mbits: row} of tests/table_rmw_ref.py, one record after the other in position order.
Nothing here knows of winner words, waves, atomics or identities, imports the library or touches a GPU.

Integers are numpy integers of the type's width: min and max compare them signed, the bitwise operations
work on the same bits.  Doubles are compared by IEEE 754 totalOrder through a sort key computed in Python
integers from the 64 bits (total_order_key); the result of a min or max is one operand's bits, copied as an
integer.  ADD delegates to tests/table_acc_ref.py."""
import struct

import numpy as np

import table_acc_ref as A

APPLIED, DROPPED, NOT_FOUND = 0, 2, 3  # DeviceTable.reduce_records' status

ADD, MIN, MAX, AND, OR, XOR = range(6)  # PDHT_RED_*
OPS = {"add": ADD, "min": MIN, "max": MAX, "and": AND, "or": OR, "xor": XOR}


def bits(x):
    """The 64 bits of the double x as a Python int."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# One of every kind of double, in totalOrder: -NaN (larger payload first) < -inf < -DBL_MAX < .. < -subnormal
# < -0.0 < +0.0 < +subnormal < .. < +DBL_MAX < +inf < +NaN (larger payload last)
QNAN, SNAN = 0x7FF8000000000001, 0x7FF0000000000001  # a quiet and a signalling payload
SIGN = 1 << 63
LADDER = [SIGN | 0x7FFFFFFFFFFFFFFF, SIGN | QNAN, SIGN | SNAN, bits(-np.inf), bits(-1.7976931348623157e308), bits(-1.5),
          bits(-2.2250738585072014e-308), SIGN | 0x000FFFFFFFFFFFFF, SIGN | 1, bits(-0.0), bits(0.0), 1,
          0x000FFFFFFFFFFFFF, bits(2.2250738585072014e-308), bits(1.5), bits(1.7976931348623157e308), bits(np.inf),
          SNAN, QNAN, 0x7FFFFFFFFFFFFFFF]


def total_order_key(bits):
    """bits: the 64 bits of a double as a Python int in 0 .. 2^64 - 1 -> an int whose order is totalOrder:
    -NaN (larger payload first) < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN (larger payload last)."""
    bits = int(bits)
    assert 0 <= bits < 1 << 64
    return bits if bits < 1 << 63 else (1 << 63) - 1 - bits  # sign set: -1 for -0.0 and down from there


def _pick(op, old, new, key):
    """min / max of two words by `key`; on equal keys the words are equal."""
    if op == MIN:
        return new if key(new) < key(old) else old
    return new if key(new) > key(old) else old


def _signed(bits, width):
    return bits - (1 << width) if bits >> (width - 1) else bits


def reduce_word(op, dtype, old, new):
    """op(old, new) on one element given as unsigned Python ints of the type's width; the result likewise."""
    dt = np.dtype(dtype)
    width = dt.itemsize * 8
    if op in (MIN, MAX):
        key = total_order_key if dt.kind == "f" else (lambda b: _signed(b, width))
        return _pick(op, old, new, key)
    assert dt.kind == "i", "and / or / xor are integer operations"
    return old & new if op == AND else old | new if op == OR else old ^ new


def replies8(state, mbits, rowbytes):
    """The head-8 replies of a get for `mbits` on `state`."""
    uniq, inv = np.unique(np.asarray(mbits, np.uint64), return_inverse=True)
    one = np.zeros((len(uniq), 8 + rowbytes), np.uint8)
    for i, k in enumerate(uniq.tolist()):
        row = state.get(k)
        if row is not None:
            one[i, 0] = 1
            one[i, 8:] = row
    return one[inv.ravel()].reshape(len(inv), 8 + rowbytes)


def reduce_ref(state, mbits, rows, dtype, op, value_offset, elems, insert, dropped=(), capacity=None):
    """Applies the batch to `state` in place.  dtype: np.int32, np.int64 or np.float64; op: ADD .. XOR or its
    name.  insert, dropped, capacity: as table_acc_ref.acc_ref.  Returns (status uint8 [m], replies uint8
    [m, 8 + rowbytes]): reply p is what a get of record p's mbits gives AFTER the call -- zeros for a record
    with status 2 or 3, which left no entry."""
    op = OPS.get(op, op)
    assert op in range(6)
    dt = np.dtype(dtype)
    mbits = np.asarray(mbits, np.uint64)
    rowbytes = np.asarray(rows).shape[1]  # rows: uint8 [m, rowbytes], also when m == 0
    if op == ADD:
        status, _ = A.acc_ref(state, mbits, rows, dtype, value_offset, elems, insert, dropped=dropped,
                              capacity=capacity)
    else:
        assert dt in (np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.float64))
        assert dt.kind == "i" or op in (MIN, MAX)
        word = np.uint32 if dt.itemsize == 4 else np.uint64
        lo, hi = value_offset, value_offset + elems * dt.itemsize
        dropped = {int(k) for k in dropped}
        status = np.zeros(len(mbits), np.uint8)
        operands = np.ascontiguousarray(np.asarray(rows)[:, lo:hi]).view(word).tolist() if len(mbits) else []
        for p, k in enumerate(mbits.tolist()):
            row = state.get(k)
            if row is None:
                if not insert:
                    status[p] = NOT_FOUND
                elif k in dropped:
                    status[p] = DROPPED
                else:
                    state[k] = np.array(rows[p], np.uint8)  # the whole row of the first record
                continue
            assert k not in dropped, "a present mbits is never dropped"
            region = row[lo:hi].view(word)  # a view: writing it writes the row
            for j, (old, new) in enumerate(zip(region.tolist(), operands[p])):
                region[j] = reduce_word(op, dt, old, new)
        if capacity is not None:
            assert sum(1 for k in state if k != 0) <= capacity
    return status, replies8(state, mbits, rowbytes)
