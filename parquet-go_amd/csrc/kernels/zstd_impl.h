// zstd_impl.h — ZSTD page decompression on the device (included by decode.hip after gzip_impl.h).
//
// The reference decompresses ZSTD blocks on the host with klauspost/compress/zstd DecodeAll
// (compress.go:79-105).  Here the pages of ZSTD chunks loaded with PQH_LOAD_DEVICE_ZSTD travel to
// HBM compressed and k_zstd rebuilds each page image, one workgroup of 256 threads per page.  The
// format's serial parts are the host decoder's own functions (zstd_core.h), so both accept and
// reject the same streams; this file is the executor:
//
//   frame / block headers, the Huffman tree and the FSE tables   lane 0 (the tables stay in LDS for
//                                                                the next block's repeat / treeless modes)
//   Huffman literals of a block                                   one lane per stream (1 or 4), into the
//                                                                page's literals scratch in HBM
//   RLE literals                                                  filled into the scratch by the workgroup
//   the FSE sequence walk                                         lane 0, into batches of elements (one
//                                                                per sequence part: literals, then match)
//   the bytes of a batch (up to kSnapOut)                         the workgroup: batch_emap finds each
//                                                                byte's element, a literal byte comes
//                                                                from the scratch (raw literals: the
//                                                                source), a match byte points inside the
//                                                                batch (batch_jump_store) or is read back
//                                                                from HBM, written by an earlier batch
//   raw / RLE blocks, literal runs of a batch or more             bulk copies / fills
//   content checksum (XXH64)                                      four lanes, one accumulator each
//
// Every index taken from the stream is checked before it is used: the walk validates each sequence
// against the block's literals, the block maximum, the page size, the frame's output so far and the
// window (PQH_ERR_DECOMPRESS); zs_batch checks each byte's source again against its buffer and
// reports PQH_ERR_INTERNAL, as k_gzip's guards do.
#pragma once

// (zstd_core.h: included by decode.hip before the namespace opens)

constexpr int kZsMaxE = 1024;  // elements per batch

// Bytes of literals scratch a ZSTD page needs: a block's literals are part of its output, so never
// more than the page's decompressed values (zs_block refuses larger ones before decoding them).
__host__ __device__ inline int64_t zstd_scratch_bytes(const pqh_codec_page& c) {
  const int64_t raw = c.raw_len < c.src_len ? c.raw_len : c.src_len;
  int64_t out = int64_t(c.image_len) - raw;
  if (out < 0) out = 0;
  if (out > int64_t(zs::kBlockMax)) out = zs::kBlockMax;
  return (out + 63) & ~int64_t(63);
}

struct __attribute__((aligned(16))) ZsLds {
  uint16_t emap[kSnapOut];     // batch resolution (batch_emap / batch_jump_store)
  uint8_t out[kSnapOut];
  int32_t eout[kZsMaxE + 1];   // element output start, batch-relative; eout[nE] = the batch size
  int32_t elp[kZsMaxE];        // where the element's literals start in the block's literals
  int32_t eoff[kZsMaxE];       // match offset
  uint16_t ell[kZsMaxE];       // literal bytes, followed by
  uint16_t eml[kZsMaxE];       // match bytes
  zs::Tables t;                // Huffman + FSE tables and repeat offsets (kept between blocks)
  zs::HufScratch hs;
  zs::SeqScratch ss;
  uint8_t weights[256];
  zs::Streams st;
  zs::Literals lit;
  zs::SeqWalk walk;
  zs::Frame frame;
  zs::Block blk;
  uint64_t xv[4];              // XXH64 lanes
  int32_t wmax[4];
  // state between phases (lane 0 writes, everyone reads after a barrier)
  int32_t ok, f_hdr, f_lit, f_seq, f_walk;
  int32_t lit_q;               // offset of the Huffman streams in the block
  int32_t nE, T, bulk_len, bulk_lp, block_done;
  uint32_t nseq, seq_left, lpos, pend_ll, pend_ml, pend_off, block_out, tail_done;
};

// Lane 0: the next batch of the current block.  Sequences are cut into elements of at most the
// room left in the batch; a literal run of a whole batch or more at a batch's start becomes a bulk
// copy.  Sets E.f_walk on a corrupt stream.
__device__ void zs_walk(ZsLds& E, uint32_t regen, uint32_t block_max, int32_t d, int32_t total, int32_t frame_start,
                        uint64_t window) {
  int32_t nE = 0, T = 0;
  E.bulk_len = 0;
  E.block_done = 0;
  for (;;) {
    if (E.pend_ll == 0 && E.pend_ml == 0) {
      if (E.seq_left == 0) {
        if (E.tail_done) {
          E.block_done = 1;
          break;
        }
        E.tail_done = 1;  // the literals after the last sequence
        if (E.nseq && E.walk.bits.left != 0) {  // the bitstream is not exactly consumed
          E.f_walk = 1;
          break;
        }
        const uint32_t tail = regen - E.lpos;
        if (E.block_out + tail > block_max || int64_t(d) + T + tail > total) {
          E.f_walk = 1;
          break;
        }
        E.block_out += tail;
        E.pend_ll = tail;
        E.pend_off = 1;
        continue;
      }
      uint32_t ll, ml, off;
      if (!zs::seq_next(&E.walk, &E.t, &ll, &ml, &off)) {
        E.f_walk = 1;
        break;
      }
      E.seq_left--;
      const int64_t at = int64_t(d) + T + ll;  // where the match starts in the page's output
      if (ll > regen - E.lpos || uint64_t(E.block_out) + ll + ml > block_max || at + ml > total ||
          off > uint64_t(at - frame_start) || off > window) {
        E.f_walk = 1;
        break;
      }
      E.block_out += ll + ml;
      E.pend_ll = ll;
      E.pend_ml = ml;
      E.pend_off = off;
    }
    const uint32_t room = uint32_t(kSnapOut - T);
    if (room == 0 || nE == kZsMaxE) break;
    if (E.pend_ll >= uint32_t(kSnapOut)) {  // a long literal run: a bulk copy of its own
      if (T == 0) {
        E.bulk_len = int32_t(E.pend_ll);
        E.bulk_lp = int32_t(E.lpos);
        E.lpos += E.pend_ll;
        E.pend_ll = 0;
      }
      break;
    }
    const uint32_t a = E.pend_ll < room ? E.pend_ll : room;
    uint32_t b = 0;
    if (a == E.pend_ll) b = E.pend_ml < room - a ? E.pend_ml : room - a;
    E.eout[nE] = T;
    E.elp[nE] = int32_t(E.lpos);
    E.ell[nE] = uint16_t(a);
    E.eml[nE] = uint16_t(b);
    E.eoff[nE] = int32_t(E.pend_off);
    nE++;
    T += int32_t(a + b);
    E.lpos += a;
    E.pend_ll -= a;
    E.pend_ml -= b;
  }
  E.eout[nE] = T;
  E.nE = nE;
  E.T = T;
}

// The workgroup: the batch's T bytes at dst[d, d + T).  lit[0, regen) are the block's literals.
// False, with nothing read or written out of bounds, when the batch's tables are inconsistent (the
// walk validated every sequence, so this is an internal error, never a corrupt page).
__device__ bool zs_batch(ZsLds& E, int32_t T, int32_t nE, int32_t d, int32_t total, const uint8_t* lit, int32_t regen,
                         uint8_t* dst) {
  const int tid = threadIdx.x;
  if (T < 1 || T > kSnapOut || nE < 1 || nE > kZsMaxE || int64_t(d) + T > total) return false;
  bool oob = false;
  batch_emap(E, nE, 0);
  int16_t ptr[kPer];
  uint8_t val[kPer];
#pragma unroll
  for (int i0 = 0; i0 < kPer; i0 += 8) {
    int32_t ga[8];
    uint8_t from[8];  // 0 in-batch pointer, 1 dst (an earlier batch), 2 the literals
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int32_t b = (i0 + j) * kBlock + tid;
      from[j] = 0;
      ga[j] = 0;
      val[i0 + j] = 0;
      ptr[i0 + j] = -1;
      if (b >= T) continue;
      const int e = E.emap[b];
      if (e >= nE) {
        oob = true;
        continue;
      }
      const int32_t rel = b - E.eout[e], ll = E.ell[e];
      if (rel < 0) {
        oob = true;
      } else if (rel < ll) {
        from[j] = 2;
        ga[j] = E.elp[e] + rel;
      } else {
        const int32_t r2 = rel - ll, ml = E.eml[e], o = E.eoff[e];
        if (r2 >= ml || o < 1) {
          oob = true;
          continue;
        }
        const int32_t sabs = d + E.eout[e] + ll - o + (o < ml ? r2 % o : r2);  // overlapping matches repeat
        if (sabs >= d) {
          if (sabs - d >= b) oob = true;  // a pointer reaches back, always
          else ptr[i0 + j] = int16_t(sabs - d);
        } else {
          from[j] = 1;
          ga[j] = sabs;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (!from[j]) continue;
      if (ga[j] < 0 || ga[j] >= (from[j] == 1 ? d : regen)) {
        oob = true;
        continue;
      }
      val[i0 + j] = from[j] == 1 ? dst[ga[j]] : lit[ga[j]];
    }
  }
  if (__syncthreads_or(oob)) return false;
  batch_jump_store(E, T, ptr, val, dst + d);
  return true;
}

// One compressed block p[0, size) appended at dst + d.  Whole workgroup; uniform result.
__device__ int zs_block(const uint8_t* p, int32_t size, uint64_t window, uint8_t* dst, int32_t& d, int32_t total,
                        int32_t frame_start, uint8_t* scratch, int32_t scratch_len, ZsLds& E) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    int bad = 0;
    E.f_lit = E.f_seq = E.f_walk = 0;
    E.lit_q = 0;
    if (!zs::literals_header(p, size, window, &E.lit)) {
      bad = 1;
    } else if (int64_t(E.lit.regen) > int64_t(total) - d || (E.lit.type != 0 && int64_t(E.lit.regen) > scratch_len)) {
      bad = 1;  // more literals than the page has room for
    } else if (E.lit.type >= 2) {
      const uint8_t* q = p + E.lit.header;
      uint32_t rem = E.lit.comp;
      if (E.lit.type == 2) {
        int count = 0;
        const int used = zs::huf_read_weights(q, rem, E.weights, &count, &E.hs);
        E.t.huf_log = -1;
        if (used < 0 || !zs::huf_build(E.weights, count, E.t.huf, &E.t.huf_log)) {
          bad = 1;
        } else {
          q += used;
          rem -= uint32_t(used);
        }
      } else if (E.t.huf_log < 0) {
        bad = 1;  // treeless with no table yet
      }
      if (!bad && !zs::split_streams(q, rem, E.lit.regen, E.lit.streams, &E.st)) bad = 1;
      E.lit_q = int32_t(q - p);
    }
    E.f_hdr = bad;
  }
  __syncthreads();
  if (uni(E.f_hdr)) return PQH_ERR_DECOMPRESS;
  const int32_t ltype = uni(int32_t(E.lit.type)), regen = uni(int32_t(E.lit.regen));
  const int32_t lhdr = uni(int32_t(E.lit.header)), lcomp = uni(int32_t(E.lit.comp));
  const uint8_t* lit = scratch;
  if (ltype == 0) {
    lit = p + lhdr;  // raw literals are read where they lie (inside the block: literals_header)
  } else if (ltype == 1) {
    const uint8_t v = p[lhdr];
    for (int32_t i = tid; i < regen; i += kBlock) scratch[i] = v;
  } else if (tid < int(uni(int32_t(E.lit.streams)))) {
    // stream tid: src inside the block (split_streams), dst inside [0, regen) <= scratch_len
    const zs::Streams& s = E.st;
    if (uint64_t(s.dst[tid]) + s.out[tid] > uint64_t(regen) ||
        !zs::huf_stream(p + E.lit_q + s.src[tid], s.len[tid], E.t.huf, E.t.huf_log, scratch + s.dst[tid], s.out[tid]))
      E.f_lit = 1;
  }
  __syncthreads();
  if (uni(E.f_lit)) return PQH_ERR_DECOMPRESS;
  if (tid == 0) {
    const uint8_t* sp = p + lhdr + lcomp;
    const int64_t sn = int64_t(size) - lhdr - lcomp;
    uint32_t nseq = 0;
    const int at = zs::seq_header(sp, sn, &E.t, &nseq, &E.ss);
    int bad = at < 0;
    if (!bad && nseq) bad = !zs::seq_begin(&E.walk, &E.t, sp + at, sn - at, nseq);
    E.nseq = E.seq_left = nseq;
    E.lpos = E.pend_ll = E.pend_ml = E.block_out = E.tail_done = 0;
    E.pend_off = 1;
    E.f_seq = bad;
  }
  __syncthreads();
  if (uni(E.f_seq)) return PQH_ERR_DECOMPRESS;
  const uint32_t block_max = window < zs::kBlockMax ? uint32_t(window) : uint32_t(zs::kBlockMax);
  for (;;) {
    if (tid == 0) zs_walk(E, uint32_t(regen), block_max, d, total, frame_start, window);
    __syncthreads();
    if (uni(E.f_walk)) return PQH_ERR_DECOMPRESS;
    const int32_t bl = uni(E.bulk_len), T = uni(E.T);
    const int32_t done = uni(E.block_done);
    if (bl > 0) {
      const int32_t lp = uni(E.bulk_lp);
      if (lp < 0 || int64_t(lp) + bl > regen || int64_t(d) + bl > total) return PQH_ERR_INTERNAL;  // (validated by zs_walk)
      snap_copy(dst + d, lit + lp, bl);
      d += bl;
    } else if (T > 0) {
      if (!zs_batch(E, T, uni(E.nE), d, total, lit, regen, dst)) return PQH_ERR_INTERNAL;
      d += T;
    } else if (!done) {
      return PQH_ERR_INTERNAL;  // no progress
    }
    __syncthreads();  // this batch's bytes are visible to the next batches' reads; the element tables are free
    if (done) break;
  }
  return PQH_OK;
}

// Decode the frames src[0, n) into dst[0, expected).  Whole workgroup; returns PQH_OK,
// PQH_ERR_DECOMPRESS or PQH_ERR_INTERNAL (uniform).
__device__ int zstd_stream(const uint8_t* src, int64_t n64, uint8_t* dst, int64_t expected, uint8_t* scratch,
                           int32_t scratch_len, ZsLds& E) {
  const int tid = threadIdx.x;
  if (n64 < 0 || expected < 0 || n64 > 0x7fffffff || expected > 0x7fffffff) return PQH_ERR_DECOMPRESS;
  const int32_t n = uni(int32_t(n64)), total = uni(int32_t(expected));
  int32_t in = 0, d = 0;
  while (in < n) {
    __syncthreads();
    if (tid == 0) {
      E.ok = zs::frame_header(src + in, uint64_t(n - in), &E.frame);
      zs::tables_reset(&E.t);
    }
    __syncthreads();
    if (!uni(E.ok)) return PQH_ERR_DECOMPRESS;
    const int32_t hdr = uni(int32_t(E.frame.header_size));
    if (hdr < 0 || hdr > n - in) return PQH_ERR_INTERNAL;  // (validated by frame_header)
    in += hdr;
    if (uni(int32_t(E.frame.skippable))) continue;
    const uint64_t window = E.frame.window;
    const int32_t frame_start = d;
    for (;;) {
      __syncthreads();
      if (tid == 0) E.ok = n - in >= 3 && zs::block_header(src + in, window, &E.blk);
      __syncthreads();
      if (!uni(E.ok)) return PQH_ERR_DECOMPRESS;
      in += 3;
      const int32_t type = uni(int32_t(E.blk.type)), size = uni(int32_t(E.blk.size)), last = uni(int32_t(E.blk.last));
      if (size < 0 || size > int32_t(zs::kBlockMax)) return PQH_ERR_INTERNAL;  // (validated by block_header)
      if (type == 0) {
        if (n - in < size || total - d < size) return PQH_ERR_DECOMPRESS;
        snap_copy(dst + d, src + in, size);
        in += size;
        d += size;
      } else if (type == 1) {
        if (n - in < 1 || total - d < size) return PQH_ERR_DECOMPRESS;
        const uint8_t v = src[in];
        for (int32_t i = tid; i < size; i += kBlock) dst[d + i] = v;
        in += 1;
        d += size;
      } else {
        if (n - in < size) return PQH_ERR_DECOMPRESS;
        const int rc = zs_block(src + in, size, window, dst, d, total, frame_start, scratch, scratch_len, E);
        if (rc != PQH_OK) return rc;
        in += size;
      }
      if (last) break;
    }
    __syncthreads();  // the frame's output is visible to the checksum lanes
    if (uni(int32_t(E.frame.has_size)) && uint64_t(d - frame_start) != E.frame.content_size) return PQH_ERR_DECOMPRESS;
    if (uni(int32_t(E.frame.checksum))) {
      if (n - in < 4) return PQH_ERR_DECOMPRESS;
      const uint8_t* fp = dst + frame_start;
      const int32_t len = d - frame_start;
      if (tid < 4) {  // XXH64: lane k owns accumulator k, the k-th 8 bytes of every 32-byte stripe
        uint64_t v[4];
        zs::xxh_init(v);
        uint64_t acc = v[tid];
        for (int32_t i = 0; i + 32 <= len; i += 32) acc = zs::xxh_round(acc, zs::le64(fp + i + 8 * tid));
        E.xv[tid] = acc;
      }
      __syncthreads();
      if (tid == 0) E.ok = zs::le32(src + in) == uint32_t(zs::xxh_finish(E.xv, fp, uint64_t(len)));
      __syncthreads();
      if (!uni(E.ok)) return PQH_ERR_DECOMPRESS;
      in += 4;
    }
  }
  return d == total ? PQH_OK : PQH_ERR_DECOMPRESS;
}

// One workgroup per ZSTD page (other codecs: k_snappy / k_gzip): its image rebuilt at image_offset.
// lits_off[page] = where the page's literals scratch starts in `lits` (zstd_scratch_bytes each).
__global__ __launch_bounds__(256) void k_zstd(const pqh_codec_page* cps, const uint8_t* src_all, uint8_t* dst_all,
                                              int32_t* status, const int64_t* lits_off, uint8_t* lits) {
  __shared__ ZsLds E;
  const pqh_codec_page cp = cps[blockIdx.x];
  if (cp.codec != PQH_CODEC_ZSTD) return;
  const uint8_t* src = src_all + cp.src_offset;
  uint8_t* dst = dst_all + cp.image_offset;
  int rc;
  const int32_t raw = cp.raw_len < cp.src_len ? cp.raw_len : cp.src_len;
  snap_copy(dst, src, raw < cp.image_len ? raw : cp.image_len);  // DataPageV2 levels: never compressed
  if (raw > cp.image_len || raw < 0) rc = PQH_ERR_DECOMPRESS;
  else rc = zstd_stream(src + raw, cp.src_len - raw, dst + raw, int64_t(cp.image_len) - raw, lits + lits_off[blockIdx.x],
                        int32_t(zstd_scratch_bytes(cp)), E);
  if (threadIdx.x == 0) status[blockIdx.x] = rc;
}
