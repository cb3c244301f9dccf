"""Plain numpy statement of the packed-row form of the 1 Mpx store (data.Gen4PackedStore, eas_count_rows_measure / _pack / _unpack,
eas_packed_store_frames).  It is this project's own definition: the reference has no such store; what ties the store to the reference is
tests/golden/gen4_store.npz and the equality of its frames with ``count_store_frames``, which that fixture pins.

A row is one sensor row of one polarity of one representation, rows in the order [R][2][H].  A row is cut into G = ceil(W / 16) <= 64 groups
of 16 pixels (pixels at and behind W count as zero).  A group is zero (all sums 0: nothing stored), narrow (maximum <= 255: 16 bytes, one
per pixel, pixel order) or wide (sixteen little-endian u16).  Table int64 [R, 2, H, 3] = (nz, wide, offset) as bit patterns: bit g of nz =
group g is not zero, bit g of wide = group g is wide, offset = the row's first unit of 16 bytes in the payload.  The groups of a row lie back
to back in ascending g, the rows follow each other in row order without gaps."""
import numpy as np

UNIT = 16
MAX_W = 1024


def groups_of(sums):
    """int64 [rows, G, 16]: every row of u16 sums [n, 2, H, W] cut into groups, zero behind W"""
    sums = np.asarray(sums)
    assert sums.dtype == np.uint16 and sums.ndim == 4 and sums.shape[1] == 2
    n, _, H, W = sums.shape
    if W > MAX_W:
        raise ValueError(f'W = {W}: more than 64 groups')
    G = (W + 15) // 16
    padded = np.zeros((n * 2 * H, G * 16), dtype=np.int64)
    padded[:, :W] = sums.reshape(n * 2 * H, W)
    return padded.reshape(n * 2 * H, G, 16)


def encode(sums, unit_offset=0):
    """(table int64 [n, 2, H, 3], payload uint8 [16 * units]) of u16 sums [n, 2, H, W]; the first row starts at unit ``unit_offset``"""
    n, _, H, W = np.asarray(sums).shape
    grp = groups_of(sums)
    table = np.zeros((grp.shape[0], 3), dtype=np.uint64)
    out, unit = [], int(unit_offset)
    for r, row in enumerate(grp):
        nz = wide = 0
        start = unit
        for g, px in enumerate(row):
            top = int(px.max())
            if top == 0:
                continue
            nz |= 1 << g
            if top <= 255:
                out.append(px.astype(np.uint8).tobytes())
                unit += 1
            else:
                wide |= 1 << g
                out.append(px.astype('<u2').tobytes())
                unit += 2
        table[r, 0], table[r, 1], table[r, 2] = np.uint64(nz), np.uint64(wide), np.uint64(start)          # (bit 63 stays a bit)
    payload = np.frombuffer(b''.join(out), dtype=np.uint8).copy()
    assert len(payload) == UNIT * (unit - int(unit_offset))
    return table.view(np.int64).reshape(n, 2, H, 3), payload


def popcount(v):
    return bin(int(v)).count('1')


def decode(table, payload, W, unit_offset=0):
    """u16 sums [n, 2, H, W] from a table and the payload whose first byte is unit ``unit_offset``: every group found through
    offset + popcount(nz & below(g)) + popcount(wide & below(g))"""
    table = np.asarray(table)
    n, _, H, _ = table.shape
    G = (W + 15) // 16
    words = table.reshape(-1, 3).view(np.uint64)
    out = np.zeros((len(words), G * 16), dtype=np.uint16)
    payload = np.asarray(payload, dtype=np.uint8)
    for r, (nz, wide, offset) in enumerate(words):
        nz, wide, offset = int(nz), int(wide), int(offset)
        assert nz >> G == 0 and wide & ~nz == 0
        for g in range(G):
            if not (nz >> g) & 1:
                continue
            below = (1 << g) - 1
            at = UNIT * (offset + popcount(nz & below) + popcount(wide & below) - int(unit_offset))
            if (wide >> g) & 1:
                out[r, g * 16:g * 16 + 16] = payload[at:at + 32].view('<u2')
            else:
                out[r, g * 16:g * 16 + 16] = payload[at:at + 16]
    assert not out[:, W:].any()
    return out[:, :W].reshape(n, 2, H, W)


def fields(H, W, seed=0):
    """u16 sums [7, 2, H, W], the contents the tests pack: zeros; every pixel 255; one pixel 256; one pixel 65 025 in the last column;
    groups alternating zero / narrow / wide; seeded sparse fields at densities 0.02 and 0.3 with values up to 300"""
    rng = np.random.default_rng([seed, H, W])
    f = np.zeros((7, 2, H, W), dtype=np.uint16)
    f[1] = 255
    f[2, 1, H // 2, W // 2] = 256
    f[3, 0, H - 1, W - 1] = 65025
    for g in range((W + 15) // 16):
        cols = slice(g * 16, min(g * 16 + 16, W))
        if g % 3 == 1:
            f[4, :, :, cols] = rng.integers(0, 256, (2, H, cols.stop - cols.start))
            f[4, :, :, cols.start] = 255                                              # (never an all-zero group by chance)
        elif g % 3 == 2:
            f[4, :, :, cols] = rng.integers(0, 301, (2, H, cols.stop - cols.start))
            f[4, :, :, cols.stop - 1] = 300
    for k, density in ((5, 0.02), (6, 0.3)):
        f[k] = np.where(rng.random((2, H, W)) < density, rng.integers(1, 301, (2, H, W)), 0)
    return f


def packed_bytes(sums):
    """(payload bytes, table bytes) of u16 sums [n, 2, H, W], counted from the classes alone"""
    grp = groups_of(sums)
    top = grp.max(axis=2)
    return UNIT * (int((top > 0).sum()) + int((top > 255).sum())), 24 * grp.shape[0]
