// zstd_core.h — the serial parts of a Zstandard frame decoder, written from RFC 8878: frame and
// block headers, FSE and Huffman table construction, the Huffman literal streams, the sequence walk
// with its repeat offsets, and XXH64.  Plain functions over pointers, compiled for the host
// (host/codec.cpp: zstd_decompress) and for the device (zstd_impl.h: k_zstd), so both decoders
// accept and reject the same streams.  No dictionaries.  Where libzstd's one-shot call and the
// reference's decoder (klauspost/compress/zstd DecodeAll) disagree, this follows the reference
// (DESIGN §9 lists the cases with both citations).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZS_HD __host__ __device__ inline
#else
#define ZS_HD inline
#endif

namespace pqhip {
namespace zs {

enum : uint32_t {
  kMagic = 0xFD2FB528u,
  kSkipMagic = 0x184D2A50u,  // .. 0x184D2A5F
  kBlockMax = 128u << 10,
  kWindowMin = 1u << 10,  // reference framedec.go:39
  kHufLogMax = 11,
  kLLLogMax = 9,
  kOFLogMax = 8,
  kMLLogMax = 9,
  kLLSyms = 36,
  kOFSyms = 32,
  kMLSyms = 53,
};
static const uint64_t kWindowMax = uint64_t(1) << 29;  // reference framedec.go:43

struct FseEntry {
  uint16_t base;  // next state = base + read(nbits)
  uint8_t sym;
  uint8_t nbits;
};

// The entropy state a block may inherit from the block before it (repeat / treeless modes), and
// the three repeat offsets.  ~9.3 KiB: lives in LDS on the device.
struct Tables {
  FseEntry ll[1 << kLLLogMax];
  FseEntry of[1 << kOFLogMax];
  FseEntry ml[1 << kMLLogMax];
  uint16_t huf[1 << kHufLogMax];  // symbol | nbits << 8, indexed by the next huf_log bits
  int32_t ll_log, of_log, ml_log, huf_log;  // -1: no table yet
  uint32_t rep[3];
};

ZS_HD void tables_reset(Tables* t) {
  t->ll_log = t->of_log = t->ml_log = t->huf_log = -1;
  t->rep[0] = 1;
  t->rep[1] = 4;
  t->rep[2] = 8;
}

ZS_HD int highbit(uint32_t v) { return 31 - __builtin_clz(v); }  // v != 0

ZS_HD uint32_t le32(const uint8_t* p) {
  return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}
ZS_HD uint64_t le64(const uint8_t* p) { return uint64_t(le32(p)) | (uint64_t(le32(p + 4)) << 32); }

// ---------------------------------------------------------------------------------------------
// XXH64 (seed 0): the content checksum is its low 32 bits over the frame's output.
static const uint64_t kP1 = 11400714785074694791ull, kP2 = 14029467366897019727ull, kP3 = 1609587929392839161ull,
                      kP4 = 9650029242287828579ull, kP5 = 2870177450012600261ull;
ZS_HD uint64_t rotl64(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
ZS_HD uint64_t xxh_round(uint64_t acc, uint64_t in) { return rotl64(acc + in * kP2, 31) * kP1; }
ZS_HD uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v)) * kP1 + kP4; }
ZS_HD void xxh_init(uint64_t v[4]) {
  v[0] = kP1 + kP2;
  v[1] = kP2;
  v[2] = 0;
  v[3] = 0 - kP1;
}
// the tail: `v` holds the four lanes after the floor(n / 32) stripes of p[0, n)
ZS_HD uint64_t xxh_finish(const uint64_t v[4], const uint8_t* p, uint64_t n) {
  uint64_t h;
  if (n >= 32) {
    h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18);
    for (int i = 0; i < 4; i++) h = xxh_merge(h, v[i]);
  } else {
    h = kP5;
  }
  h += n;
  uint64_t i = n & ~uint64_t(31);
  for (; i + 8 <= n; i += 8) h = rotl64(h ^ xxh_round(0, le64(p + i)), 27) * kP1 + kP4;
  if (i + 4 <= n) {
    h = rotl64(h ^ (uint64_t(le32(p + i)) * kP1), 23) * kP2 + kP3;
    i += 4;
  }
  for (; i < n; i++) h = rotl64(h ^ (p[i] * kP5), 11) * kP1;
  h ^= h >> 33;
  h *= kP2;
  h ^= h >> 29;
  h *= kP3;
  h ^= h >> 32;
  return h;
}
ZS_HD uint64_t xxh64(const uint8_t* p, uint64_t n) {
  uint64_t v[4];
  xxh_init(v);
  for (uint64_t i = 0; i + 32 <= n; i += 32)
    for (int k = 0; k < 4; k++) v[k] = xxh_round(v[k], le64(p + i + 8 * k));
  return xxh_finish(v, p, n);
}

// ---------------------------------------------------------------------------------------------
// Frame and block headers.
struct Frame {
  uint64_t window;        // 0 for a skippable frame
  uint64_t content_size;  // valid iff has_size
  uint32_t header_size;   // bytes up to the first block (skippable: the whole frame)
  bool has_size, checksum, skippable;
};

// Parses the frame at p[0, n).  False: bad magic, truncated, a reserved bit, a dictionary, or a
// window the reference refuses.
ZS_HD bool frame_header(const uint8_t* p, uint64_t n, Frame* f) {
  if (n < 4) return false;
  const uint32_t magic = le32(p);
  f->skippable = false;
  f->has_size = f->checksum = false;
  f->window = f->content_size = 0;
  if ((magic & 0xFFFFFFF0u) == kSkipMagic) {
    if (n < 8) return false;
    const uint64_t len = le32(p + 4);
    if (len > n - 8) return false;
    f->skippable = true;
    f->header_size = uint32_t(8 + len);
    return true;
  }
  if (magic != kMagic || n < 5) return false;
  const uint8_t d = p[4];
  const bool single = (d >> 5) & 1;
  if (d & 8) return false;  // reserved bit
  f->checksum = (d >> 2) & 1;
  const int did = (d & 3) == 3 ? 4 : (d & 3);
  int fcs = d >> 6;
  fcs = fcs == 0 ? (single ? 1 : 0) : (1 << fcs);
  uint64_t at = 5;
  if (n < at + (single ? 0 : 1) + uint64_t(did) + uint64_t(fcs)) return false;
  if (!single) {
    const uint8_t w = p[at++];
    const uint64_t base = uint64_t(1) << (10 + (w >> 3));
    f->window = base + (base >> 3) * (w & 7);
  }
  uint32_t dict = 0;
  for (int i = 0; i < did; i++) dict |= uint32_t(p[at++]) << (8 * i);
  if (dict != 0) return false;  // no dictionaries
  if (fcs) {
    uint64_t v = 0;
    for (int i = 0; i < fcs; i++) v |= uint64_t(p[at++]) << (8 * i);
    if (fcs == 2) v += 256;
    f->content_size = v;
    f->has_size = true;
  }
  if (f->window > kWindowMax) return false;  // reference framedec.go:230 (ErrWindowSizeExceeded)
  if (single) f->window = f->content_size < kWindowMin ? uint64_t(kWindowMin) : f->content_size;  // framedec.go:237-242
  f->header_size = uint32_t(at);
  return true;
}

struct Block {
  uint32_t type;  // 0 raw, 1 RLE, 2 compressed
  uint32_t size;  // Block_Size: the regenerated size of an RLE block, else the bytes that follow
  bool last;
};

// The 3-byte block header at p (the caller checked 3 bytes).  False: reserved type, or a size the
// reference refuses (over 128 KiB or over the window: blockdec.go:149,169,181; a compressed block
// under 2 bytes: blockdec.go:177).
ZS_HD bool block_header(const uint8_t* p, uint64_t window, Block* b) {
  const uint32_t h = uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16);
  b->last = h & 1;
  b->type = (h >> 1) & 3;
  b->size = h >> 3;
  if (b->type == 3) return false;
  if (b->size > kBlockMax || b->size > window) return false;
  if (b->type == 2 && b->size < 2) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------
// Bit readers.  Forward (FSE distributions): little-endian bits from the first byte.  Backward
// (every entropy-coded stream): starts under the final-bit marker of the last byte.  Neither ever
// touches a byte outside [p, p + n): bits past the ends read as zero and are caught by the callers'
// "exactly consumed" checks.
ZS_HD uint64_t load_bits(const uint8_t* p, int64_t n, int64_t byte) {  // 8 bytes from p + byte, zero outside [0, n)
  uint64_t v = 0;
  if (byte >= 0 && byte + 8 <= n) {
    __builtin_memcpy(&v, p + byte, 8);
    return v;
  }
  for (int i = 0; i < 8; i++) {
    const int64_t k = byte + i;
    if (k >= 0 && k < n) v |= uint64_t(p[k]) << (8 * i);
  }
  return v;
}

struct RevBits {
  const uint8_t* p;
  int64_t n;
  int64_t left;  // bits not yet consumed; negative once over-read
};

ZS_HD bool rev_init(RevBits* r, const uint8_t* p, int64_t n) {
  if (n < 1 || p[n - 1] == 0) return false;
  r->p = p;
  r->n = n;
  r->left = 8 * (n - 1) + highbit(p[n - 1]);
  return true;
}
// the next k (0..32) bits without consuming them; bits below the start read as zero
ZS_HD uint32_t rev_peek(const RevBits* r, int k) {
  if (k == 0) return 0;
  const int64_t lo = r->left - k;
  const uint64_t mask = (uint64_t(1) << k) - 1;
  if (lo >= 0) return uint32_t((load_bits(r->p, r->n, lo >> 3) >> (lo & 7)) & mask);
  if (r->left <= 0) return 0;
  const uint64_t have = load_bits(r->p, r->n, 0) & ((uint64_t(1) << r->left) - 1);  // left < k <= 32
  return uint32_t((have << (-lo)) & mask);
}
ZS_HD uint32_t rev_read(RevBits* r, int k) {
  const uint32_t v = rev_peek(r, k);
  r->left -= k;
  return v;
}

// ---------------------------------------------------------------------------------------------
// FSE.  fse_read_dist parses a normalised distribution (RFC 8878 §4.1.1) from p[0, n) into
// norm[0, *nsym) (-1: "less than one") and returns the bytes it occupies, or -1.
ZS_HD int fse_read_dist(const uint8_t* p, int64_t n, int max_log, int max_syms, int16_t* norm, int* nsym, int* log) {
  if (n < 1) return -1;
  int64_t bit = 4;
  const int al = (p[0] & 15) + 5;
  if (al > max_log) return -1;  // accuracy log out of range
  int remaining = (1 << al) + 1, threshold = 1 << al, nbits = al + 1, s = 0;
  while (remaining > 1 && s < max_syms) {
    if ((bit >> 3) >= n) return -1;
    const uint32_t v = uint32_t(load_bits(p, n, bit >> 3) >> (bit & 7));
    const int max = (2 * threshold - 1) - remaining;
    int count;
    if (int(v & uint32_t(threshold - 1)) < max) {
      count = int(v & uint32_t(threshold - 1));
      bit += nbits - 1;
    } else {
      count = int(v & uint32_t(2 * threshold - 1));
      if (count >= threshold) count -= max;
      bit += nbits;
    }
    count--;
    remaining -= count < 0 ? -count : count;
    norm[s++] = int16_t(count);
    if (count == 0) {
      for (;;) {  // repeat flags: 2 bits each, 3 means another follows
        if ((bit >> 3) >= n) return -1;
        const int rep = int((load_bits(p, n, bit >> 3) >> (bit & 7)) & 3);
        bit += 2;
        for (int i = 0; i < rep; i++) {
          if (s >= max_syms) return -1;
          norm[s++] = 0;
        }
        if (rep != 3) break;
      }
    }
    if (remaining < 1) return -1;  // the distribution over-runs its table
    while (remaining < threshold) {
      nbits--;
      threshold >>= 1;
    }
  }
  if (remaining != 1) return -1;
  const int64_t bytes = (bit + 7) >> 3;
  if (bytes > n) return -1;
  *nsym = s;
  *log = al;
  return int(bytes);
}

// Builds the decoding table of 1 << log entries.  `next` is scratch for nsym values.
ZS_HD bool fse_build(const int16_t* norm, int nsym, int log, FseEntry* tab, uint16_t* next) {
  const int size = 1 << log;
  int high = size - 1;
  for (int s = 0; s < nsym; s++) {
    if (norm[s] == -1) {
      if (high < 0) return false;
      tab[high--].sym = uint8_t(s);
      next[s] = 1;
    } else {
      next[s] = uint16_t(norm[s]);
    }
  }
  const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
  int pos = 0;
  for (int s = 0; s < nsym; s++)
    for (int i = 0; i < norm[s]; i++) {
      if (pos > high) return false;
      tab[pos].sym = uint8_t(s);
      do pos = (pos + step) & mask;
      while (pos > high);
    }
  if (pos != 0) return false;
  for (int u = 0; u < size; u++) {
    const uint32_t x = next[tab[u].sym]++;
    const int nb = log - highbit(x);
    tab[u].nbits = uint8_t(nb);
    tab[u].base = uint16_t((x << nb) - uint32_t(size));
  }
  return true;
}

ZS_HD void fse_rle(FseEntry* tab, uint8_t sym) {
  tab[0].sym = sym;
  tab[0].nbits = 0;
  tab[0].base = 0;
}

// ---------------------------------------------------------------------------------------------
// Huffman.  huf_read_weights parses a tree description at p[0, n) into w[0, *count) (the explicit
// weights; the last one is implied) and returns the bytes it occupies, or -1.  `ws` is scratch.
struct HufScratch {
  int16_t norm[256];
  uint16_t next[256];
  FseEntry fse[64];
};

ZS_HD int huf_read_weights(const uint8_t* p, int64_t n, uint8_t* w, int* count, HufScratch* ws) {
  if (n < 1) return -1;
  const int hb = p[0];
  if (hb >= 128) {  // direct: 4 bits per weight
    const int k = hb - 127, bytes = (k + 1) / 2;
    if (1 + bytes > n) return -1;
    for (int i = 0; i < k; i++) w[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
    *count = k;
    return 1 + bytes;
  }
  if (hb == 0 || 1 + hb > n) return -1;
  int nsym, log;
  const int used = fse_read_dist(p + 1, hb, 6, 256, ws->norm, &nsym, &log);
  if (used < 0 || !fse_build(ws->norm, nsym, log, ws->fse, ws->next)) return -1;
  RevBits r;
  if (!rev_init(&r, p + 1 + used, hb - used)) return -1;
  uint32_t s1 = rev_read(&r, log), s2 = rev_read(&r, log);
  int k = 0;
  for (;;) {  // two interleaved states until the stream over-reads
    if (k > 253) return -1;
    w[k++] = ws->fse[s1].sym;
    s1 = ws->fse[s1].base + rev_read(&r, ws->fse[s1].nbits);
    if (r.left < 0) {
      w[k++] = ws->fse[s2].sym;
      break;
    }
    if (k > 253) return -1;
    w[k++] = ws->fse[s2].sym;
    s2 = ws->fse[s2].base + rev_read(&r, ws->fse[s2].nbits);
    if (r.left < 0) {
      w[k++] = ws->fse[s1].sym;
      break;
    }
  }
  *count = k;
  return 1 + hb;
}

// Builds the lookup table from count explicit weights (w has room for one more).  False: a weight
// over 11, weights that do not complete a power of two, or a tree deeper than 11 bits.
ZS_HD bool huf_build(uint8_t* w, int count, uint16_t* tab, int32_t* log) {
  uint32_t total = 0, rank[kHufLogMax + 2];
  for (uint32_t r = 0; r < kHufLogMax + 2; r++) rank[r] = 0;
  for (int i = 0; i < count; i++) {
    if (w[i] > kHufLogMax) return false;
    if (w[i]) total += 1u << (w[i] - 1);
    rank[w[i]]++;
  }
  if (total == 0) return false;
  const int bits = highbit(total) + 1;
  if (bits > int(kHufLogMax)) return false;
  const uint32_t rest = (1u << bits) - total;
  if (rest & (rest - 1)) return false;  // the last weight must complete a power of two
  w[count] = uint8_t(highbit(rest) + 1);
  rank[w[count]]++;
  count++;
  if (rank[1] < 2 || (rank[1] & 1)) return false;  // by construction (huff0/decompress.go:112)
  uint32_t start[kHufLogMax + 2], pos = 0;
  for (int r = 1; r <= bits; r++) {
    start[r] = pos;
    pos += rank[r] << (r - 1);
  }
  if (pos != (1u << bits)) return false;
  for (int s = 0; s < count; s++) {
    const int r = w[s];
    if (!r) continue;
    const uint32_t len = 1u << (r - 1);
    const uint16_t e = uint16_t(s | ((bits + 1 - r) << 8));
    for (uint32_t i = 0; i < len; i++) tab[start[r] + i] = e;
    start[r] += len;
  }
  *log = bits;
  return true;
}

// One Huffman stream src[0, n) -> dst[0, m): true iff it yields m symbols and is exactly consumed.
ZS_HD bool huf_stream(const uint8_t* src, int64_t n, const uint16_t* tab, int log, uint8_t* dst, int64_t m) {
  RevBits r;
  if (!rev_init(&r, src, n)) return false;
  for (int64_t i = 0; i < m; i++) {
    const uint16_t e = tab[rev_peek(&r, log)];  // the index has log bits: inside the table
    dst[i] = uint8_t(e);
    r.left -= e >> 8;
    if (r.left < 0) return false;
  }
  return r.left == 0;
}

// ---------------------------------------------------------------------------------------------
// Literals section header.
struct Literals {
  uint32_t type;     // 0 raw, 1 RLE, 2 compressed, 3 treeless
  uint32_t streams;  // 1 or 4 (types 2 and 3)
  uint32_t regen;    // regenerated size
  uint32_t comp;     // bytes after the header: regen (raw), 1 (RLE) or the compressed size
  uint32_t header;   // header bytes
};

// False: truncated, or sizes beyond the block / the 128 KiB block maximum / the window
// (blockdec.go:349).
ZS_HD bool literals_header(const uint8_t* p, int64_t n, uint64_t window, Literals* l) {
  if (n < 1) return false;
  const uint32_t b0 = p[0], sf = (b0 >> 2) & 3;
  l->type = b0 & 3;
  l->streams = 1;
  if (l->type < 2) {
    if ((sf & 1) == 0) {
      l->header = 1;
      l->regen = b0 >> 3;
    } else if (sf == 1) {
      if (n < 2) return false;
      l->header = 2;
      l->regen = (b0 >> 4) | (uint32_t(p[1]) << 4);
    } else {
      if (n < 3) return false;
      l->header = 3;
      l->regen = (b0 >> 4) | (uint32_t(p[1]) << 4) | (uint32_t(p[2]) << 12);
    }
    l->comp = l->type == 0 ? l->regen : 1;
  } else {
    l->header = sf < 2 ? 3 : sf + 2;
    if (n < int64_t(l->header)) return false;
    uint64_t v = 0;
    for (uint32_t i = 0; i < l->header; i++) v |= uint64_t(p[i]) << (8 * i);
    v >>= 4;
    const int bits = sf < 2 ? 10 : (sf == 2 ? 14 : 18);
    l->regen = uint32_t(v & ((1u << bits) - 1));
    l->comp = uint32_t((v >> bits) & ((1u << bits) - 1));
    l->streams = sf == 0 ? 1 : 4;
  }
  if (l->regen > kBlockMax || l->regen > window) return false;
  if (uint64_t(l->header) + l->comp > uint64_t(n)) return false;
  return true;
}

// The 4-stream split of `comp` bytes at p (after the tree description) regenerating `regen`
// bytes: offsets and lengths of stream k in the source and in the literals.
struct Streams {
  uint32_t src[4], len[4], dst[4], out[4];
};
ZS_HD bool split_streams(const uint8_t* p, uint32_t comp, uint32_t regen, uint32_t streams, Streams* s) {
  if (streams == 1) {
    s->src[0] = 0;
    s->len[0] = comp;
    s->dst[0] = 0;
    s->out[0] = regen;
    return true;
  }
  if (comp < 6) return false;
  const uint32_t l1 = p[0] | (uint32_t(p[1]) << 8), l2 = p[2] | (uint32_t(p[3]) << 8), l3 = p[4] | (uint32_t(p[5]) << 8);
  if (uint64_t(6) + l1 + l2 + l3 > comp) return false;
  const uint32_t seg = (regen + 3) / 4;
  if (3 * seg > regen) return false;
  s->src[0] = 6;
  s->len[0] = l1;
  s->src[1] = 6 + l1;
  s->len[1] = l2;
  s->src[2] = 6 + l1 + l2;
  s->len[2] = l3;
  s->src[3] = 6 + l1 + l2 + l3;
  s->len[3] = comp - s->src[3];
  for (int k = 0; k < 4; k++) {
    s->dst[k] = uint32_t(k) * seg;
    s->out[k] = k < 3 ? seg : regen - 3 * seg;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// Sequences section.
struct SeqScratch {
  int16_t norm[64];
  uint16_t next[64];
};

ZS_HD const int16_t* predefined(int which, int* nsym, int* log) {
  static const int16_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  static const int16_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  static const int16_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  if (which == 0) {
    *nsym = 36;
    *log = 6;
    return ll;
  }
  if (which == 1) {
    *nsym = 29;
    *log = 5;
    return of;
  }
  *nsym = 53;
  *log = 6;
  return ml;
}

// One of the three tables (which: 0 LL, 1 OF, 2 ML) in `mode`, its description at p[0, n).
// Returns the bytes consumed, or -1.
ZS_HD int seq_table(int which, int mode, const uint8_t* p, int64_t n, FseEntry* tab, int32_t* log, SeqScratch* ws) {
  const int max_log = which == 0 ? kLLLogMax : (which == 1 ? kOFLogMax : kMLLogMax);
  const int max_syms = which == 0 ? kLLSyms : (which == 1 ? kOFSyms : kMLSyms);
  if (mode == 0) {
    int nsym, lg;
    const int16_t* d = predefined(which, &nsym, &lg);
    for (int i = 0; i < nsym; i++) ws->norm[i] = d[i];
    if (!fse_build(ws->norm, nsym, lg, tab, ws->next)) return -1;
    *log = lg;
    return 0;
  }
  if (mode == 1) {
    if (n < 1 || p[0] >= max_syms) return -1;
    fse_rle(tab, p[0]);
    *log = 0;
    return 1;
  }
  if (mode == 2) {
    int nsym, lg;
    const int used = fse_read_dist(p, n, max_log, max_syms, ws->norm, &nsym, &lg);
    if (used < 0 || !fse_build(ws->norm, nsym, lg, tab, ws->next)) return -1;
    *log = lg;
    return used;
  }
  return *log < 0 ? -1 : 0;  // repeat: needs a table from an earlier block of this frame
}

// The sequences section at p[0, n): count, the three tables, then the bitstream.  Returns the
// offset of the bitstream, or -1; *nseq == 0 means the section must end right after its count.
ZS_HD int seq_header(const uint8_t* p, int64_t n, Tables* t, uint32_t* nseq, SeqScratch* ws) {
  if (n < 1) return -1;
  int at = 1;
  uint32_t c = p[0];
  if (c >= 128) {
    if (c == 255) {
      if (n < 3) return -1;
      c = (uint32_t(p[1]) | (uint32_t(p[2]) << 8)) + 0x7F00;
      at = 3;
    } else {
      if (n < 2) return -1;
      c = ((c - 128) << 8) | p[1];
      at = 2;
    }
  }
  *nseq = c;
  if (c == 0) return at == n ? at : -1;
  if (n < at + 1) return -1;
  const int modes = p[at++];
  if (modes & 3) return -1;  // reserved
  int u = seq_table(0, modes >> 6, p + at, n - at, t->ll, &t->ll_log, ws);
  if (u < 0) return -1;
  at += u;
  u = seq_table(1, (modes >> 4) & 3, p + at, n - at, t->of, &t->of_log, ws);
  if (u < 0) return -1;
  at += u;
  u = seq_table(2, (modes >> 2) & 3, p + at, n - at, t->ml, &t->ml_log, ws);
  if (u < 0) return -1;
  at += u;
  return at;
}

ZS_HD void ll_code(uint32_t c, uint32_t* base, uint32_t* bits) {
  static const uint32_t b[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,   10,  11,  12,   13,   14,   15,   16,    18,
                                 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
  static const uint8_t e[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  *base = b[c];
  *bits = e[c];
}
ZS_HD void ml_code(uint32_t c, uint32_t* base, uint32_t* bits) {
  static const uint32_t b[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13,  14,  15,  16,   17,   18,   19,   20,
                                 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,  32,  33,  34,   35,   37,   39,   41,
                                 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
  static const uint8_t e[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  *base = b[c];
  *bits = e[c];
}

struct SeqWalk {
  RevBits bits;
  uint32_t ll, of, ml;  // FSE states
  uint32_t left;        // sequences still to decode
};

ZS_HD bool seq_begin(SeqWalk* w, const Tables* t, const uint8_t* p, int64_t n, uint32_t nseq) {
  if (!rev_init(&w->bits, p, n)) return false;
  w->ll = rev_read(&w->bits, t->ll_log);
  w->of = rev_read(&w->bits, t->of_log);
  w->ml = rev_read(&w->bits, t->ml_log);
  w->left = nseq;
  return w->bits.left >= 0;
}

// The next sequence: literal length, match length and the resolved match offset (the repeat
// offsets in t->rep are updated).  False: an over-read stream or a symbol outside its alphabet.
// After the last sequence the caller checks w->bits.left == 0.
ZS_HD bool seq_next(SeqWalk* w, Tables* t, uint32_t* lit, uint32_t* match, uint32_t* offset) {
  const FseEntry le = t->ll[w->ll], oe = t->of[w->of], me = t->ml[w->ml];
  if (le.sym >= kLLSyms || oe.sym >= kOFSyms || me.sym >= kMLSyms) return false;
  uint32_t lb, lx, mb, mx;
  ll_code(le.sym, &lb, &lx);
  ml_code(me.sym, &mb, &mx);
  const uint32_t ov = (1u << oe.sym) + rev_read(&w->bits, oe.sym);
  *match = mb + rev_read(&w->bits, int(mx));
  *lit = lb + rev_read(&w->bits, int(lx));
  uint32_t* rep = t->rep;
  uint32_t off;
  if (ov > 3) {
    off = ov - 3;
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = off;
  } else {
    const uint32_t idx = ov + (*lit == 0 ? 1 : 0);  // 1..4
    if (idx == 1) {
      off = rep[0];
    } else {
      off = idx == 4 ? rep[0] - 1 : rep[idx - 1];
      if (off == 0) off = 1;  // corrupt input: both decoders force 1
      if (idx != 2) rep[2] = rep[1];
      rep[1] = rep[0];
      rep[0] = off;
    }
  }
  *offset = off;
  if (--w->left) {  // no state update after the last sequence
    w->ll = le.base + rev_read(&w->bits, le.nbits);
    w->ml = me.base + rev_read(&w->bits, me.nbits);
    w->of = oe.base + rev_read(&w->bits, oe.nbits);
  }
  return w->bits.left >= 0;
}

}  // namespace zs
}  // namespace pqhip
