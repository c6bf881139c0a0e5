"""ZSTD page blocks for the codec tests (helper, no tests): pyarrow-compressed samples that together
reach every feature of the format (RFC 8878), a header parser that names the features a stream
uses, frames assembled byte by byte for the frame-level cases, the cases where libzstd and the
reference's decoder differ (fixed expectations), seeded mutants, and a corpus dump for the
stand-alone driver (csrc/tools/zstd_check.cpp).  Cases are (name, stream, page size)."""
import struct

import numpy as np
import pyarrow as pa

LEVELS = (-5, 1, 3, 9, 19)
MAGIC = b"\x28\xb5\x2f\xfd"


# ---------------------------------------------------------------------------------------------
# samples
def url_lines(n, seed=0):
    rng = np.random.default_rng(seed)
    hosts = [b"example.com", b"data.example.org", b"cdn.static.net", b"api.service.io"]
    paths = [b"index", b"item", b"user/profile", b"search", b"cart/checkout"]
    a, b, c = rng.integers(0, 4, n), rng.integers(0, 5, n), rng.integers(0, 1 << 20, n)
    return b"".join(b"https://%s/%s?id=%d&ref=%d\n" % (hosts[a[i]], paths[b[i]], c[i], c[i] % 97) for i in range(n))


def samples(seed=11):
    rng = np.random.default_rng(seed)

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    first = rnd(200000)
    zipf = np.minimum(rng.zipf(1.3, 200000) - 1, 255).astype(np.uint8).tobytes()
    return [
        ("empty", b""),
        ("three", b"abc"),
        ("text", (b"the quick brown fox jumps over the lazy dog; " * 5)[:200]),
        ("sym3", rng.integers(0, 3, 1000, dtype=np.uint8).tobytes()),
        ("const", b"\x07" * 500000),
        ("random", rnd(300000)),
        ("urls", url_lines(30000, seed)),
        ("rep8", np.repeat(rng.integers(0, 1 << 62, 30000, dtype=np.int64), 8).tobytes()),
        ("sym4", (rng.integers(0, 4, 400000, dtype=np.uint8) + 65).astype(np.uint8).tobytes()),
        ("zipf", zipf),
        ("cumsum", np.cumsum(rng.integers(0, 1000, 150000, dtype=np.int64)).tobytes()),
        ("rand-x-rand", rnd(70000) + b"x" * 300000 + rnd(1000)),
        ("far-match", first + rnd(1200000) + first),
        # (a 14th sample: with this generator none of the 13 above makes pyarrow emit RLE literals)
        ("flags", np.random.default_rng(seed).integers(0, 2, 50000, dtype=np.int64).tobytes()),
    ]


_CACHE = {}


def compressed(levels=LEVELS, seed=11):
    """[(name, stream, size)]: every sample at every level."""
    key = (tuple(levels), seed)
    if key not in _CACHE:
        out = []
        for name, raw in samples(seed):
            for lv in levels:
                s = pa.Codec("zstd", compression_level=lv).compress(raw, asbytes=True)
                out.append((f"{name}-L{lv}", s, len(raw)))
        _CACHE[key] = out
    return _CACHE[key]


def raw_of(name, seed=11):
    return dict(samples(seed))[name.rsplit("-L", 1)[0]]


# ---------------------------------------------------------------------------------------------
# features
def features(stream):
    """The set of format features `stream` (valid frames) uses, from its headers alone."""
    f, at, n = set(), 0, len(stream)
    while at < n:
        magic = struct.unpack_from("<I", stream, at)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            f.add("skippable")
            at += 8 + struct.unpack_from("<I", stream, at + 4)[0]
            continue
        assert stream[at:at + 4] == MAGIC
        d = stream[at + 4]
        at += 5
        single = (d >> 5) & 1
        f.add("single-segment" if single else "windowed")
        if d & 4:
            f.add("checksum")
        if not single:
            at += 1
        at += (0, 1, 2, 4)[d & 3]
        fcs = (1 if single else 0, 2, 4, 8)[d >> 6]
        f.add(f"fcs{fcs}")
        at += fcs
        while True:
            h = stream[at] | (stream[at + 1] << 8) | (stream[at + 2] << 16)
            at += 3
            last, typ, size = h & 1, (h >> 1) & 3, h >> 3
            f.add(("block-raw", "block-rle", "block-compressed")[typ])
            if typ == 2:
                _block_features(stream[at:at + size], f)
            at += 1 if typ == 1 else size
            if last:
                break
        if d & 4:
            at += 4
    return f


def _block_features(b, f):
    typ, sf = b[0] & 3, (b[0] >> 2) & 3
    f.add(("lit-raw", "lit-rle", "lit-huffman", "lit-treeless")[typ])
    if typ < 2:
        hdr = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
        regen = int.from_bytes(b[:hdr], "little") >> (3 if hdr == 1 else 4)
        at = hdr + (regen if typ == 0 else 1)
    else:
        hdr = 3 if sf < 2 else sf + 2
        bits = 10 if sf < 2 else (14 if sf == 2 else 18)
        v = int.from_bytes(b[:hdr], "little") >> 4
        comp = (v >> bits) & ((1 << bits) - 1)
        f.add("streams1" if sf == 0 else "streams4")
        if typ == 2:
            f.add("weights-direct" if b[hdr] >= 128 else "weights-fse")
        at = hdr + comp
    c = b[at]
    at += 1
    if c == 0:
        f.add("seq0")
        return
    f.add("seq-count1" if c < 128 else ("seq-count2" if c < 255 else "seq-count3"))
    at += 0 if c < 128 else (1 if c < 255 else 2)
    modes = b[at]
    for name, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        f.add(f"{name}-" + ("predefined", "rle", "fse", "repeat")[(modes >> shift) & 3])


REQUIRED_FEATURES = frozenset(
    ["single-segment", "windowed", "fcs1", "fcs2", "fcs4", "block-raw", "block-rle", "block-compressed",
     "lit-raw", "lit-rle", "lit-huffman", "lit-treeless", "streams1", "streams4", "weights-direct",
     "weights-fse", "seq0"] + [f"{t}-{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")])


# ---------------------------------------------------------------------------------------------
# XXH64 (seed 0) in pure Python, for checksummed frames
_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161,
                           9650029242287828579, 2870177450012600261)


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & _M


def _round(acc, x):
    return (_rotl((acc + x * _P2) & _M, 31) * _P1) & _M


def xxh64(data):
    n, i = len(data), 0
    if n >= 32:
        v = [(_P1 + _P2) & _M, _P2, 0, (-_P1) & _M]
        words = np.frombuffer(data[:n & ~31], dtype="<u8").tolist()
        for j in range(0, len(words), 4):
            for k in range(4):
                v[k] = _round(v[k], words[j + k])
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = (((h ^ _round(0, v[k])) * _P1) + _P4) & _M
        i = n & ~31
    else:
        h = _P5
    h = (h + n) & _M
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[i:i + 8], "little")), 27) * _P1 + _P4) & _M
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h = (_rotl(h ^ (data[i] * _P5 & _M), 11) * _P1) & _M
        i += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    h ^= h >> 32
    return h


def with_checksum(stream, raw, good=True):
    """A single pyarrow frame with descriptor bit 2 set and the 4 checksum bytes appended."""
    c = xxh64(raw) & 0xFFFFFFFF
    if not good:
        c ^= 0x10000
    return stream[:4] + bytes([stream[4] | 4]) + stream[5:] + struct.pack("<I", c)


# ---------------------------------------------------------------------------------------------
# hand-built frames
def block(typ, payload, size=None, last=False):
    """typ 0 raw / 1 RLE (payload: the one byte, size: the run) / 2 compressed / 3 reserved."""
    size = len(payload) if size is None else size
    return struct.pack("<I", (size << 3) | (typ << 1) | int(last))[:3] + payload


def frame(blocks, fcs=None, fcs_bytes=None, window=None, dict_id=None, dict_bytes=0, checksum=None, reserved=False):
    """window: the window descriptor byte (None: single segment).  fcs_bytes 0 needs a window."""
    single = window is None
    if fcs_bytes is None:
        fcs_bytes = 1 if single else 0
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    d = (flag << 6) | (int(single) << 5) | (8 if reserved else 0) | (4 if checksum is not None else 0)
    d |= {0: 0, 1: 1, 2: 2, 4: 3}[dict_bytes]
    out = MAGIC + bytes([d])
    if not single:
        out += bytes([window])
    out += (dict_id or 0).to_bytes(dict_bytes, "little")
    if fcs_bytes:
        out += ((fcs - 256) if fcs_bytes == 2 else fcs).to_bytes(fcs_bytes, "little")
    out += b"".join(blocks)
    if checksum is not None:
        out += struct.pack("<I", checksum)
    return out


def skippable(payload, nibble=3):
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


def hand_built():
    """Frame-level cases both decoders agree on (the oracle decides what is expected)."""
    a, b = b"hello, frame! " * 3, bytes(range(200, 256)) * 6
    fa = frame([block(0, a, last=True)], fcs=len(a))
    fb = frame([block(0, b[:100]), block(1, b"z", 50), block(0, b[100:], last=True)], fcs=len(b) + 50, fcs_bytes=2)
    raw300 = bytes(range(256)) + bytes(44)
    urls = url_lines(400, 5)
    zurls = pa.Codec("zstd", compression_level=3).compress(urls, asbytes=True)
    out = [
        ("empty-input-empty-page", b"", 0),
        ("empty-input-page", b"", 5),
        ("skippable-alone", skippable(b"meta"), 0),
        ("skippable-empty", skippable(b"", 0), 0),
        ("skippable-then-frame", skippable(b"1234567", 15) + fa, len(a)),
        ("frame-then-skippable", fa + skippable(b"x"), len(a)),
        ("frame-frame", fa + fb, len(a) + len(b) + 50),
        ("frame-pyarrow-frame", fa + zurls + fa, 2 * len(a) + len(urls)),
        ("three-blocks-fcs2", fb, len(b) + 50),
        ("fcs2-raw300", frame([block(0, raw300, last=True)], fcs=300, fcs_bytes=2), 300),
        ("fcs4", frame([block(0, a, last=True)], fcs=len(a), fcs_bytes=4), len(a)),
        ("fcs8", frame([block(0, a, last=True)], fcs=len(a), fcs_bytes=8), len(a)),
        ("windowed-no-size", frame([block(0, a), block(1, b"q", 1000, last=True)], window=0x10), len(a) + 1000),
        ("windowed-fcs4", frame([block(0, a, last=True)], fcs=len(a), fcs_bytes=4, window=0x08), len(a)),
        ("empty-raw-block", frame([block(0, b"", last=True)], fcs=0), 0),
        ("rle-0", frame([block(1, b"r", 0), block(0, a, last=True)], fcs=len(a)), len(a)),
        ("rle-128k", frame([block(1, b"r", 131072, last=True)], fcs=131072, fcs_bytes=4), 131072),
        ("dict-id-0-1byte", frame([block(0, a, last=True)], fcs=len(a), dict_id=0, dict_bytes=1), len(a)),
        ("dict-id-0-4byte", frame([block(0, a, last=True)], fcs=len(a), dict_id=0, dict_bytes=4), len(a)),
        ("dict-id-7", frame([block(0, a, last=True)], fcs=len(a), dict_id=7, dict_bytes=1), len(a)),
        ("dict-id-2byte", frame([block(0, a, last=True)], fcs=len(a), dict_id=300, dict_bytes=2), len(a)),
        ("reserved-bit", frame([block(0, a, last=True)], fcs=len(a), reserved=True), len(a)),
        ("fcs-mismatch-short", frame([block(0, a, last=True)], fcs=len(a) + 1), len(a)),
        ("fcs-mismatch-long", frame([block(0, a, last=True)], fcs=len(a) - 1), len(a)),
        ("no-last-block", frame([block(0, a)], fcs=len(a)), len(a)),
        ("trailing-byte", fa + b"\0", len(a)),
        ("trailing-magic", fa + MAGIC, len(a)),
        ("block-type-3", frame([block(3, a, last=True)], fcs=len(a)), len(a)),
        ("raw-block-truncated", frame([block(0, a, size=len(a) + 4, last=True)], fcs=len(a) + 4), len(a) + 4),
        ("bad-magic", b"\x29" + fa[1:], len(a)),
        ("page-smaller", fa, len(a) - 1),
        ("checksum-good-raw", frame([block(0, a, last=True)], fcs=len(a), checksum=xxh64(a) & 0xFFFFFFFF), len(a)),
        ("checksum-bad-raw", frame([block(0, a, last=True)], fcs=len(a), checksum=(xxh64(a) + 1) & 0xFFFFFFFF), len(a)),
        ("checksum-missing", frame([block(0, a, last=True)], fcs=len(a), checksum=0)[:-4], len(a)),
        ("checksum-good-pyarrow", with_checksum(zurls, urls), len(urls)),
        ("checksum-bad-pyarrow", with_checksum(zurls, urls, good=False), len(urls)),
    ]
    big = raw_of("urls")[:70000]
    zbig = pa.Codec("zstd", compression_level=1).compress(big, asbytes=True)
    out.append(("checksum-good-70k", with_checksum(zbig, big), len(big)))
    return out


def reference_cases():
    """[(name, stream, size, expected bytes or None, citation)]: where libzstd's one-shot call and the
    reference's DecodeAll differ, the decoder follows the reference (vendored klauspost/compress/zstd)."""
    r2000 = bytes(i % 251 for i in range(2000))
    r1024 = r2000[:1024]
    return [
        ("raw-block-over-window", frame([block(0, r2000, last=True)], window=0x00), 2000, None, "blockdec.go:181"),
        ("rle-block-over-window", frame([block(1, b"w", 2000, last=True)], window=0x00), 2000, None, "blockdec.go:149"),
        ("raw-block-fills-window", frame([block(0, r1024, last=True)], window=0x00), 1024, r1024, "blockdec.go:181"),
        ("window-1gib", frame([block(0, b"abc", last=True)], window=(20 << 3)), 3, None, "framedec.go:43,230"),
        ("window-512mib", frame([block(0, b"abc", last=True)], window=(19 << 3)), 3, b"abc", "framedec.go:43,230"),
        ("compressed-block-1-byte", frame([block(2, b"\0", last=True)], fcs=0), 0, None, "blockdec.go:177"),
        ("compressed-block-0-bytes", frame([block(2, b"", last=True)], fcs=0), 0, None, "blockdec.go:177"),
    ]


# ---------------------------------------------------------------------------------------------
# mutants
def mutants(valid, seed=7, per=9):
    """Seeded corruptions of valid streams: one to three byte overwrites, a truncation, a bit flip
    (page size kept).  Bytes 4 and 5, the frame header descriptor and the window descriptor (or the
    first content-size byte), are never touched: the hand-built cases cover them, and libzstd and
    the reference differ on window sizes (reference_cases)."""
    rng = np.random.default_rng(seed)
    out = []
    for name, s, size in valid:
        for k in range(per):
            b = bytearray(s)
            mode = k % 3
            if mode == 0:
                for _ in range(int(rng.integers(1, 4))):
                    b[int(rng.integers(6, len(b)))] = int(rng.integers(0, 256))
            elif mode == 1:
                b = b[:int(rng.integers(6, len(b)))]
            else:
                b[int(rng.integers(6, len(b)))] ^= 1 << int(rng.integers(0, 8))
            out.append((f"{name}-mut{k}", bytes(b), size))
    return out


def mutant_corpus():
    return mutants([c for c in compressed() if c[0].endswith(("-L1", "-L19"))])


# ---------------------------------------------------------------------------------------------
# corpus dump for the stand-alone driver: "ZSTC", u32 count, then per case u32 name length, name,
# u32 stream length, stream, u64 page size, u32 valid, and the expected bytes when valid
def dump_corpus(path, cases):
    """cases: [(name, stream, size, expected bytes or None)]."""
    with open(path, "wb") as fh:
        fh.write(b"ZSTC" + struct.pack("<I", len(cases)))
        for name, s, size, want in cases:
            nm = name.encode()
            fh.write(struct.pack("<I", len(nm)) + nm + struct.pack("<I", len(s)) + s)
            fh.write(struct.pack("<QI", size, int(want is not None)))
            if want is not None:
                assert len(want) == size
                fh.write(want)
