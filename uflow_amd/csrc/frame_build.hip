// frame_build.hip -- batched Frame::write on device-resident records: the send-side mirror of
// frame_parse.hip (ufc_build_sizes_varlen / ufc_build_batch_varlen, include/uflow_frame_codec.h).
//
// The encode itself is frame_codec_core.hpp (shared with the host build, frame_codec.cpp): write_* of
// src/frame/serial/mod.rs:437-657, DataFrameBuilder of build.rs:55-162 and AckFrameBuilder of :192-247.
//
// Sizes (one launch + one scan):
//   1. check: one thread per frame -> its status and encoded size (a data frame's thread walks its
//      <= 127 item records), the size stored into out_offsets[i];
//   2. scan:  hipcub exclusive sum in place over the n + 1 lengths -> out_offsets.
// Write (three launches + one scan; nothing is taken from a sizes call):
//   1. item sizes: one thread per item -> its encoded size as a datagram (header form + payload);
//   2. scan:  exclusive sum over the n_items + 1 sizes -> every item's destination, relative to the
//      first item's (a frame's datagram k starts 6 + dst[item_first + k] - dst[item_first] bytes into
//      the frame, whatever other frames do with the item array);
//   3. check: as above, and one flag byte per frame: written or not (status OK and the span given in
//      out_offsets has the frame's size and lies inside the batch's range and the buffer);
//   4. write: output-stationary.  The batch's bytes are one contiguous stream; each lane owns aligned
//      16-byte pieces of it (by address, so every full piece is one aligned 16-byte store whatever
//      the alignment of d_out_bytes).  A workgroup covers kSpanBytes of the stream and stages in LDS the
//      offsets, flags and infos of the frames that touch its span and the destinations of their items;
//      a lane finds its frame there (binary search), then its item (binary search over the item
//      destinations), and assembles its piece in registers
//      from header bytes (packed words of the core), payload bytes (one unaligned 16-byte load placed
//      so that the bytes fall where they go; byte loads at the payload buffer's two ends) and the zero
//      trailer.  Whole pieces are stored non-temporally; pieces that hold bytes of a frame that is not
//      written, or lie at the batch's two ragged ends, store their bytes one by one.
// This keeps every store a full aligned 16 bytes per lane, 1 KiB contiguous per wave (DESIGN.md section
// 5.3 measured sub-64-byte scattered writes as read-modify-writes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "frame_build.hpp"
#include "frame_build_piece.hpp"
#include "frame_codec_core.hpp"
#include "scan.hpp"

namespace ufc_dev {

namespace {

__global__ __launch_bounds__(kBuildThreads) void build_item_sizes_kernel(const ufc_item* items, uint64_t n_items,
                                                                          uint64_t* dst) {
  const uint64_t g = (uint64_t)blockIdx.x * kBuildThreads + threadIdx.x;
  if (g < n_items)
    dst[g] = ufc_codec::datagram_encoded_size(items[g]);
  else if (g == n_items)
    dst[g] = 0;
}

// kWrite false: lengths into out_offsets (scanned next) and statuses.  kWrite true: the write flags,
// against the offsets the caller gave.
// The write also records, for every workgroup span of the write kernel, the frame that owns the span's
// first byte (span_owner[s], s <= spans): the frames find the span starts inside them, so the write's
// workgroups start from one load, not from a binary search over all offsets.
template <bool kWrite>
__global__ __launch_bounds__(kBuildThreads) void build_check_kernel(BuildArgs a, uint8_t* flags, uint32_t* span_owner,
                                                                    uint64_t spans) {
  const uint64_t i = (uint64_t)blockIdx.x * kBuildThreads + threadIdx.x;
  if (i > a.n) return;
  if (i == a.n) {
    if (!kWrite) a.out_offsets[i] = 0;
    return;
  }
  uint64_t size;
  const uint8_t st =
      ufc_codec::check_frame(a.infos[i], a.items, a.n_items, a.src_base ? a.src_base[i] : 0ull, a.payload_len, size);
  if (kWrite) {
    const uint64_t oa = a.out_offsets[i], ob = a.out_offsets[i + 1], lo = a.out_offsets[0];
    flags[i] = ufc_codec::span_matches(st, size, oa, ob, lo, a.out_offsets[a.n], a.out_len) ? 1 : 0;
    note_span_owner((uint64_t)(uintptr_t)a.out_bytes, lo, oa, ob, (uint32_t)i, span_owner, spans);
  } else {
    a.out_offsets[i] = size;
    if (a.status) a.status[i] = st;
  }
}

__global__ __launch_bounds__(kBuildThreads) void build_write_kernel(BuildArgs a, const uint64_t* dst,
                                                                    const uint8_t* flags, const uint32_t* span_owner) {
  __shared__ uint64_t tab[kTabFrames + 1];
  __shared__ ufc_frame_info sinfo[kTabFrames];
  __shared__ uint8_t sflag[kTabFrames];
  __shared__ uint64_t sdst[kTabItems + 1];
  __shared__ uint32_t s_item_lo, s_item_hi;
  const uint32_t t = threadIdx.x;
  const uint32_t n = (uint32_t)a.n;
  const uint64_t* __restrict__ off = a.out_offsets;
  const uint64_t lo = off[0], hi = min(off[n], a.out_len);
  if (hi <= lo) return;
  // Pieces by address: the stream [lo, hi) of out_bytes, cut at multiples of 16 of the address.
  const uint64_t base = (uint64_t)(uintptr_t)a.out_bytes;
  const uint64_t addr_lo = base + lo, addr_hi = base + hi;
  const uint64_t span0 = first_span_addr(addr_lo) + (uint64_t)blockIdx.x * kSpanBytes;
  if (span0 >= addr_hi) return;
  const uint64_t span1 = span0 + kSpanBytes;
  // The frames that may own bytes of the span: from the owner of its first byte to the owner of the next
  // span's first byte (the check kernel's span_owner; clamped, and every lane verifies the frame it
  // finds, so offsets that are out of order leave bytes unwritten and nothing else).
  const uint32_t f_a = min(span_owner[blockIdx.x], n - 1);
  const uint32_t f_b = span1 < addr_hi ? max(f_a, min(span_owner[blockIdx.x + 1], n - 1)) : n - 1;
  const uint32_t nf = f_b - f_a + 1;
  const bool staged = UFC_BUILD_FRAMES_STAGED(nf);
  if (t == 0) {
    s_item_lo = 0xFFFFFFFFu;
    s_item_hi = 0;
  }
  __syncthreads();
  if (staged) {
    for (uint32_t j = t; j <= nf; j += kBuildThreads) tab[j] = off[f_a + j];
    for (uint32_t j = t; j < nf; j += kBuildThreads) {
      const ufc_frame_info info = a.infos[f_a + j];
      const uint8_t fl = flags[f_a + j];
      sinfo[j] = info;
      sflag[j] = fl;
      // (a written data frame: item_first + item_count <= n_items, checked by the check kernel)
      if (fl && info.kind == UFC_FRAME_DATA && info.item_count) {
        atomicMin(&s_item_lo, info.item_first);  // (LDS atomics)
        atomicMax(&s_item_hi, info.item_first + info.item_count);
      }
    }
  }
  __syncthreads();
  const uint32_t item_lo = s_item_lo, item_hi = s_item_hi;
  const bool items_staged = UFC_BUILD_ITEMS_STAGED(staged, item_lo, item_hi);
  if (items_staged)
    for (uint32_t j = t; j <= item_hi - item_lo; j += kBuildThreads) sdst[j] = dst[item_lo + j];
  __syncthreads();
  const SpanTables tb{tab, sinfo, sflag, sdst, GlobalTables{off, flags, a.infos, dst}, f_a, item_lo, staged, items_staged};

  for (int r = 0; r < kPiecesPerLane; r++) {
    const uint64_t addr = span0 + ((uint64_t)r * kBuildThreads + t) * kPiece;
    const uint64_t pa = max(addr, addr_lo), pb = min(addr + kPiece, addr_hi);
    if (pa >= pb) continue;
    Piece pc;
    assemble_piece(a, tb, f_a, f_b, addr, pa, pb, pc);
    if (pc.set == 0xFFFFu) {
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      u64x2 v;
      v.x = pc.w0;
      v.y = pc.w1;
      __builtin_nontemporal_store(v, (__attribute__((address_space(1))) u64x2*)(uintptr_t)addr);
    } else {
      uint8_t* q = (uint8_t*)(uintptr_t)addr;
      for (uint32_t j = 0; j < kPiece; j++)
        if (pc.set & (1u << j)) q[j] = (uint8_t)pc.byte(j);
    }
  }
}

}  // namespace

hipError_t build_sizes(const BuildArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  const size_t temp_bytes = scan_temp_bytes<uint64_t>(a.n + 1);
  char* temp;
  hipError_t e = scratch.get(temp_bytes, &temp);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((a.n + 1 + kBuildThreads - 1) / kBuildThreads);
  build_check_kernel<false><<<blocks, kBuildThreads, 0, stream>>>(a, nullptr, nullptr, 0);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return exclusive_sum(temp, temp_bytes, a.out_offsets, a.out_offsets, a.n + 1, stream);
}

hipError_t build_write(const BuildArgs& a, const ScratchSource& scratch, hipStream_t stream) {
  // One workgroup per kSpanBytes of the buffer's first out_len bytes (the batch's stream lies inside them;
  // a workgroup past its end returns after reading the two end offsets).
  const uint64_t wblocks = write_spans(a.out_len);
  const size_t temp_bytes = scan_temp_bytes<uint64_t>(a.n_items + 1);
  ScratchPlan plan;  // the items' destination offsets, a flag byte per frame, a word per span, the scan's temporaries
  const uint64_t at_dst = plan.take((a.n_items + 1) * 8);
  const uint64_t at_flags = plan.take(a.n);
  const uint64_t at_owners = plan.take((wblocks + 1) * 4);
  const uint64_t at_temp = plan.take(temp_bytes);
  char* s;
  hipError_t e = scratch.get(plan.end, &s);
  if (e != hipSuccess) return e;
  if (wblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (a.out_len == 0) return hipSuccess;  // no frame fits: nothing is written
  uint64_t* dst = (uint64_t*)(s + at_dst);
  uint8_t* flags = (uint8_t*)(s + at_flags);
  uint32_t* owners = (uint32_t*)(s + at_owners);
  const unsigned iblocks = (unsigned)((a.n_items + 1 + kBuildThreads - 1) / kBuildThreads);
  build_item_sizes_kernel<<<iblocks, kBuildThreads, 0, stream>>>(a.items, a.n_items, dst);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = exclusive_sum(s + at_temp, temp_bytes, dst, dst, a.n_items + 1, stream)) != hipSuccess) return e;
  const unsigned fblocks = (unsigned)((a.n + 1 + kBuildThreads - 1) / kBuildThreads);
  build_check_kernel<true><<<fblocks, kBuildThreads, 0, stream>>>(a, flags, owners, wblocks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  build_write_kernel<<<(unsigned)wblocks, kBuildThreads, 0, stream>>>(a, dst, flags, owners);
  return hipGetLastError();
}

}  // namespace ufc_dev
