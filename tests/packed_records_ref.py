"""Numpy statement of the packed records (include/eas_hip.h; ``ops.records_pack`` / ``ops.records_unpack``, ``data.Gen1PackedWindowStore``):
the field widths, the kind of every block, pack, unpack and the byte count, in plain loops over blocks -- and seeded records that hold a
block of every kind the format distinguishes.  Records are rows (t, word) of ``uint32``: the two little-endian words of a .dat record,
word = x | y << 14 | p << 28."""
import numpy as np

BLOCK, UNIT = 64, 256


def widths(H, W):
    """(XB, YB, DB); ValueError where fewer than 8 bits are left for the time"""
    xb, yb = max(int(W - 1).bit_length(), 1), max(int(H - 1).bit_length(), 1)
    if 31 - xb - yb < 8 or H > 16384 or W > 16384 or H < 1 or W < 1:
        raise ValueError(f'{H} x {W}: {31 - xb - yb} bits for the time')
    return xb, yb, 31 - xb - yb


def padded(rec):
    """the records in whole blocks [NB, 64, 2]: behind the last record, copies of it"""
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 2)
    nb = (len(rec) + BLOCK - 1) // BLOCK
    if nb == 0:
        return rec.reshape(0, BLOCK, 2)
    return np.concatenate([rec, np.repeat(rec[-1:], nb * BLOCK - len(rec), axis=0)]).reshape(nb, BLOCK, 2)


def block_kinds(rec, H, W):
    """(base uint32 [NB]: the minimum time of every block, wide bool [NB])"""
    xb, yb, db = widths(H, W)
    blocks = padded(rec)
    base, wide = np.zeros(len(blocks), dtype=np.uint32), np.zeros(len(blocks), dtype=bool)
    for b, blk in enumerate(blocks):
        t, word = blk[:, 0].astype(np.int64), blk[:, 1].astype(np.int64)
        base[b] = t.min()
        x, y = word & 16383, (word >> 14) & 16383
        wide[b] = not ((x < (1 << xb)).all() and (y < (1 << yb)).all() and ((word >> 29) == 0).all() and (t - t.min() < (1 << db)).all())
    return base, wide


def pack(rec, H, W, unit_offset=0):
    """(table uint32 [NB, 2] = (base, unit | wide << 31), payload uint8: the units of THIS call, i.e. the arena from byte ``unit_offset`` *
    256 on)"""
    xb, yb, _ = widths(H, W)
    blocks = padded(rec)
    base, wide = block_kinds(rec, H, W)
    table, parts, unit = np.zeros((len(blocks), 2), dtype=np.uint32), [], int(unit_offset)
    for b, blk in enumerate(blocks):
        table[b] = base[b], unit | (int(wide[b]) << 31)
        if wide[b]:
            parts.append(blk.astype('<u4').tobytes())
        else:
            t, word = blk[:, 0].astype(np.int64), blk[:, 1].astype(np.int64)
            x, y, p = word & 16383, (word >> 14) & 16383, (word >> 28) & 1
            parts.append((x | (y << xb) | (p << (xb + yb)) | ((t - int(base[b])) << (xb + yb + 1))).astype('<u4').tobytes())
        unit += 2 if wide[b] else 1
    return table, np.frombuffer(b''.join(parts), dtype=np.uint8).copy()


def unpack(table, payload, a, e, H, W, unit_offset=0):
    """logical records [a, e) as rows (t, word); ``payload`` as ``pack`` returns it"""
    xb, yb, _ = widths(H, W)
    words = np.asarray(payload, dtype=np.uint8).view('<u4').astype(np.int64)
    out = np.zeros((e - a, 2), dtype=np.uint32)
    for i in range(a, e):
        base, second = int(table[i // BLOCK, 0]), int(table[i // BLOCK, 1])
        first = ((second & 0x7fffffff) - unit_offset) * (UNIT // 4)
        if second >> 31:
            out[i - a] = words[first + 2 * (i % BLOCK)], words[first + 2 * (i % BLOCK) + 1]
        else:
            w = int(words[first + i % BLOCK])
            x, y, p = w & ((1 << xb) - 1), (w >> xb) & ((1 << yb) - 1), (w >> (xb + yb)) & 1
            out[i - a] = (base + (w >> (xb + yb + 1))) & 0xffffffff, x | (y << 14) | (p << 28)
    return out


def packed_bytes(rec, H, W):
    """(payload bytes, table bytes)"""
    _, wide = block_kinds(rec, H, W)
    return UNIT * (len(wide) + int(wide.sum())), 8 * len(wide)


# ------------------------------------------------------------------------------------------------ records of every kind
def word(x, y, p):
    return (np.asarray(x, dtype=np.int64) | (np.asarray(y, dtype=np.int64) << 14) | (np.asarray(p, dtype=np.int64) << 28)).astype(np.uint32)


KINDS = ('random', 'span_max', 'span_over', 'x_top', 'x_over', 'bit29', 'backwards', 'equal', 'y_over', 'y_top', 'outside')
WIDE = dict(random=False, span_max=False, span_over=True, x_top=False, x_over=True, bit29=True, backwards=False, equal=False, y_over=True,
            y_top=False, outside=None)             # None: wide exactly when the sensor's sides are powers of two (see ``kind_block``)


def kind_block(kind, H, W, t0, rng):
    """one block [64, 2] of the kind named, its times from ``t0`` on"""
    xb, yb, db = widths(H, W)
    x, y, p = rng.integers(0, W, BLOCK), rng.integers(0, H, BLOCK), rng.integers(0, 2, BLOCK)
    t = t0 + np.sort(rng.integers(0, min(1 << db, 5000), BLOCK))
    extra = np.zeros(BLOCK, dtype=np.int64)
    if kind == 'span_max':                          # exactly 2^DB - 1 us between the earliest and the latest record: narrow
        t[0], t[-1] = t0, t0 + (1 << db) - 1
    elif kind == 'span_over':                       # 2^DB: wide
        t[0], t[-1] = t0, t0 + (1 << db)
    elif kind == 'x_top':                           # the largest x a narrow block holds (outside the sensor unless W is a power of two)
        x[17] = (1 << xb) - 1
    elif kind == 'x_over':
        x[17] = 1 << xb
    elif kind == 'y_top':
        y[40] = (1 << yb) - 1
    elif kind == 'y_over':
        y[40] = 1 << yb
    elif kind == 'bit29':
        extra[5] = 1 << 29
    elif kind == 'backwards':                       # time steps backwards inside the block: the base is the minimum, not the first time
        t = np.r_[t[32:], t[:32]]
    elif kind == 'equal':
        t[:] = t0 + 7
    elif kind == 'outside':                         # events just outside the sensor: inside the fields unless the side is a power of two
        x[3], y[9] = W, H
    return np.stack([t.astype(np.uint32), word(x, y, p) | extra.astype(np.uint32)], axis=1)


def records_of_every_kind(H, W, n=None, seed=0):
    """(records uint32 [n, 2], kinds): blocks of every kind of ``KINDS`` in turn, each 20 ms behind the one in front, repeated until ``n``
    records are there (default: one round); times stay far below 2^32"""
    rng = np.random.default_rng(seed)
    n = len(KINDS) * BLOCK if n is None else int(n)
    blocks, kinds, t0 = [], [], 1_000_000
    while len(blocks) * BLOCK < n:
        kind = KINDS[len(blocks) % len(KINDS)]
        blocks.append(kind_block(kind, H, W, t0, rng))
        kinds.append(kind)
        t0 += 20_000
    return np.concatenate(blocks)[:n], kinds


def expected_wide(kinds, H, W):
    xb, yb, _ = widths(H, W)
    outside_wide = W == 1 << xb or H == 1 << yb
    return np.array([outside_wide if WIDE[k] is None else WIDE[k] for k in kinds], dtype=bool)


def as_bytes(rec):
    return np.ascontiguousarray(rec, dtype='<u4').view(np.uint8).reshape(-1)
