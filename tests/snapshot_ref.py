"""Plain numpy / standard-library restatement of what a store snapshot is checked by, shared by tests/test_cpu_store_snapshot.py and
tests/test_gpu_store_snapshot.py; nothing here imports ``eas_snn_amd``.

``digest``: the 128-bit digest of include/eas_hip.h (``eas_bytes_digest``), word by word with Python integers for short inputs and with
numpy for long ones -- the two agree, and the five known answers of the definition are ``KNOWN``.  ``read_snapshot``: an independent
reader of the file layout of DESIGN section 3l -- the magic ``EASSTORE``, a uint32 format version, a uint64 header length, a JSON header,
the sections as raw little-endian bytes on 4096-byte boundaries."""
import json
import struct

import numpy as np

MASK = (1 << 64) - 1
GOLDEN, M1, M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MAGIC, VERSION, ALIGN = b'EASSTORE', 1, 4096
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097]           # the tail word, the 16-byte pairing and a single block


def _as_bytes(buf):
    return buf.tobytes() if isinstance(buf, np.ndarray) else bytes(buf)


def digest_slow(buf):
    """(sum, xor) by the definition, one word at a time with Python integers"""
    raw = _as_bytes(buf)
    raw += bytes(-len(raw) % 8)
    s = x = 0
    for i in range(len(raw) // 8):
        z = (int.from_bytes(raw[8 * i:8 * i + 8], 'little') + (i + 1) * GOLDEN) & MASK
        z = ((z ^ (z >> 30)) * M1) & MASK
        z = ((z ^ (z >> 27)) * M2) & MASK
        z ^= z >> 31
        s, x = (s + z) & MASK, x ^ z
    return s, x


def digest(buf):
    """(sum, xor) by the definition, vectorised (uint64 arithmetic wraps mod 2^64)"""
    raw = _as_bytes(buf)
    q = np.frombuffer(raw + bytes(-len(raw) % 8), dtype='<u8').astype(np.uint64)
    if len(q) == 0:
        return 0, 0
    z = q + np.arange(1, len(q) + 1, dtype=np.uint64) * np.uint64(GOLDEN)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
    z = z ^ (z >> np.uint64(31))
    return int(np.add.reduce(z, dtype=np.uint64)), int(np.bitwise_xor.reduce(z))


def known_inputs():
    return [b'', b'\x01', bytes(range(256)), bytes(17), np.random.default_rng(0).integers(0, 256, 4097, dtype=np.uint8).tobytes()]


KNOWN = [(0x0, 0x0), (0x910a2dec89025cc1, 0x910a2dec89025cc1), (0x0308856e007df973, 0xe6ad80d5f91ad8ef),
         (0x575da3bc9ce078f2, 0x8a9c6b4b5aaded14), (0x1ac49c5ccbff564a, 0x7c581dc73ad5b3b8)]


def random_bytes(n, seed=0):
    return np.random.default_rng([seed, n]).integers(0, 256, n, dtype=np.uint8)


def read_snapshot(path):
    """(header dict, {section name: numpy array}) of a snapshot file, with every rule of the layout asserted on the way: magic, version,
    header inside the file, sections 4096-aligned, inside the file, not overlapping, of the byte length their dtype and shape take, and
    of the digest the header states"""
    raw = open(path, 'rb').read()
    assert raw[:8] == MAGIC
    version, length = struct.unpack('<IQ', raw[8:20])
    assert version == VERSION and 20 + length <= len(raw)
    header = json.loads(raw[20:20 + length].decode('utf-8'))
    arrays, end = {}, 20 + length
    for e in header['sections']:
        assert e['where'] in ('host', 'device') and e['name'] not in arrays
        dtype = np.dtype(e['dtype'])
        assert e['nbytes'] == int(np.prod(e['shape'], dtype=np.int64)) * dtype.itemsize
        part = b''
        if e['nbytes']:
            assert e['offset'] % ALIGN == 0 and e['offset'] >= end and e['offset'] + e['nbytes'] <= len(raw), e
            end = e['offset'] + e['nbytes']
            part = raw[e['offset']:end]
        assert [f'0x{w:016x}' for w in digest(part)] == e['digest'], e['name']
        arrays[e['name']] = np.frombuffer(part, dtype=dtype).reshape(e['shape'])
    return header, arrays
