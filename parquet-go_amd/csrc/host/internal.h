// internal.h — host structures shared by the C-ABI implementation files.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "pqhip.h"

struct pqh_host_batch {
  std::vector<pqh_chunk> chunks;
  std::vector<pqh_page> pages;
  // page images (or device-codec source bytes), 64-byte aligned (a packed chunk's pages after its
  // first: back to back, see plain_value_size), PQH_PAYLOAD_PAD zero bytes at the end: plain host memory, or (pqh_file_load_pinned) a block of the context's pinned pool, shared
  // with the staged batches created from it and returned to the pool when the last holder lets go
  std::shared_ptr<uint8_t> buf;
  size_t buf_size = 0;           // pad included
  bool pinned = false;
  int64_t payload_bytes = 0;     // without the pad
  const uint8_t* data() const { return buf.get(); }
  size_t size() const { return buf_size; }
  double decompress_seconds = 0;
  // device codecs (PQH_LOAD_DEVICE_SNAPPY): payload holds the SOURCE bytes of every page, and
  // codec_pages[i] rebuilds page i's image at pages[i].image_offset of an image buffer of
  // image_bytes (+ PQH_PAYLOAD_PAD)
  std::vector<pqh_codec_page> codec_pages;
  int64_t image_bytes = 0;
};

namespace pqhip {
// A block of at least `bytes` pinned host memory from the context's pool (nullptr on failure); the
// block goes back to the pool when the returned pointer's last holder releases it.
std::shared_ptr<uint8_t> pinned_acquire(pqh_ctx* ctx, size_t bytes);

// getValuesDecoder (chunk_reader.go:106-159) resolved to a kernel kind; value bytes per output value.
int32_t resolve_kind(int32_t physical_type, int32_t type_length, int32_t encoding, int32_t* value_size);

// Bytes per value of a column whose PLAIN page images are its decoded values as they stand (the
// walker packs such chunks, the batch hands them out in place: pqh_chunk_out.values), 0 for every
// other type: not BOOLEAN (bit-packed), not INT96 (a short last value is the reference's nil).
inline int32_t plain_value_size(const pqh_column& c) {
  switch (c.physical_type) {
    case PQH_INT32: case PQH_FLOAT: return 4;
    case PQH_INT64: case PQH_DOUBLE: return 8;
    case PQH_FIXED_LEN_BYTE_ARRAY: return c.type_length > 0 ? c.type_length : 0;
    default: return 0;
  }
}
}  // namespace pqhip
