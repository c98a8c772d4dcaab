// FLAC decoding for gfx950 (nppc_audio/flac.py; specification tests/flac_ref.py).  The decoder itself
// is csrc/flac_core.h, shared with the host entry points below and with tools/check/flac_host_check.cc.
//   nppc_flac_probe / nppc_flac_decode_host   host only: STREAMINFO, and the serial decoder (frame after frame)
//   nppc_flac_scan     every byte position of a batch of files tested for a frame header; 16 bytes per lane, one 16-byte
//                      load plus the byte after them, so a header may straddle any lane's or workgroup's range
//   nppc_flac_parse    one lane per candidate: the frame parsed to its end with stores off
//   nppc_flac_chain    one lane per file: the serial decoder's walk over the parsed candidates (hash lookup by offset)
//   nppc_flac_decode   one lane per accepted frame, writing where its own header says
// A frame is a serial bit parse, so the lanes of a wave walk different frames: their loop counts diverge and their loads
// and stores are strided by whole frames (served by the L2, not coalesced).  Workgroups are one wave, so a slow frame holds
// back 63 others at most.  The only atomics are an integer append counter and the 64-bit compare-and-swap of the hash
// insert; no result depends on their order.
#include "common.h"
#include "flac_core.h"
#include "nppc_hip.h"

namespace {

constexpr int META = NPPC_FLAC_META;
constexpr int HDR = 8;                       // longs in front of the candidate arrays; [0] = candidate counter

struct Work {
  unsigned long long* counter;
  long* cand_off;                            // global byte offset of the candidate
  long* cand_end;                            // byte offset, within its file, just past the frame
  unsigned long long* hkeys;                 // global byte offset + 1; 0 = empty
  int* cand_res;                             // status of the parse
  int* accepted;
  int* cand_file;
  int* hvals;                                // candidate index
  long cap, hsize;
  int hshift;
};

long hash_size(long cap, int* shift) {
  long h = 64;
  int lg = 6;
  while (h < 2 * cap) h <<= 1, ++lg;
  *shift = 64 - lg;
  return h;
}

long work_longs(long cap) {
  int sh;
  const long h = hash_size(cap, &sh);
  return HDR + 2 * cap + h + (3 * cap + h + 1) / 2;
}

Work carve(long* work, long cap) {
  Work w;
  w.cap = cap;
  w.hsize = hash_size(cap, &w.hshift);
  w.counter = reinterpret_cast<unsigned long long*>(work);
  w.cand_off = work + HDR;
  w.cand_end = w.cand_off + cap;
  w.hkeys = reinterpret_cast<unsigned long long*>(w.cand_end + cap);
  w.cand_res = reinterpret_cast<int*>(w.hkeys + w.hsize);
  w.accepted = w.cand_res + cap;
  w.cand_file = w.accepted + cap;
  w.hvals = w.cand_file + cap;
  return w;
}

__device__ __forceinline__ FlacInfo load_info(const long* __restrict__ m) {
  FlacInfo si;
  si.rate = (int)m[2], si.channels = (int)m[3], si.bps = (int)m[4], si.min_bs = (int)m[5], si.max_bs = (int)m[6];
  si.total = m[7], si.first_frame = m[8];
  return si;
}

__device__ __forceinline__ long hash_slot(const Work& w, long g) {
  return (long)(((unsigned long long)g * 0x9E3779B97F4A7C15ull) >> w.hshift);
}

// candidate index of the header at global byte offset g; -1 when there is none
__device__ int hash_find(const Work& w, long g) {
  long s = hash_slot(w, g);
  for (long n = 0; n < w.hsize; ++n) {
    const unsigned long long k = w.hkeys[s];
    if (k == 0) return -1;
    if (k == (unsigned long long)g + 1) return w.hvals[s];
    s = (s + 1) & (w.hsize - 1);
  }
  return -1;
}

// ----------------------------------------------------------------------------------------------------------------- scan
__device__ void scan_test(const unsigned char* __restrict__ bytes, const long* __restrict__ meta, int nfiles, const Work& w,
                          long g) {
  int lo = 0, hi = nfiles - 1;                                   // the last file with byte_begin <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (meta[(long)mid * META] <= g) lo = mid;
    else hi = mid - 1;
  }
  const long* m = meta + (long)lo * META;
  const long begin = m[0], size = m[1] - m[0], rel = g - begin;
  if (rel < 0 || rel >= size) return;
  const FlacInfo si = load_info(m);
  if (rel < si.first_frame) return;                              // metadata: no frame chain can pass through here
  FlacFrame fr;
  if (flac_parse_header(bytes + begin, size, rel, si, &fr) != NPPC_FLAC_OK) return;
  const unsigned long long idx = atomicAdd(w.counter, 1ull);
  if (idx >= (unsigned long long)w.cap) return;                  // counted; the chain kernel reports the overflow
  w.cand_off[idx] = g;
  w.cand_file[idx] = lo;
  long s = hash_slot(w, g);
  for (long n = 0; n < w.hsize; ++n) {                           // at most cap of hsize >= 2 cap slots are ever taken
    if (atomicCAS(&w.hkeys[s], 0ull, (unsigned long long)g + 1) == 0ull) {
      w.hvals[s] = (int)idx;
      return;
    }
    s = (s + 1) & (w.hsize - 1);
  }
}

__global__ __launch_bounds__(256) void flac_scan_kernel(const unsigned char* __restrict__ bytes, long total,
                                                        const long* __restrict__ meta, int nfiles, Work w, int aligned) {
  const long nvec = (total + 15) >> 4;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long)gridDim.x * 256) {
    const long base = v << 4;
    unsigned char b[17];
    if (aligned && base + 16 <= total) {
      const uint4 u = *reinterpret_cast<const uint4*>(bytes + base);
      const unsigned q[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) b[k] = (unsigned char)(q[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) b[k] = base + k < total ? bytes[base + k] : 0;
    }
    b[16] = base + 16 < total ? bytes[base + 16] : 0;
    unsigned hits = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) hits |= (unsigned)(b[k] == 0xff && (b[k + 1] & 0xfe) == 0xf8) << k;
    while (hits) {
      const int k = __ffs(hits) - 1;
      hits &= hits - 1;
      scan_test(bytes, meta, nfiles, w, base + k);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- parse
__global__ __launch_bounds__(64) void flac_parse_kernel(const unsigned char* __restrict__ bytes, const long* __restrict__ meta,
                                                        Work w) {
  const unsigned long long found = *w.counter;
  const long n = found < (unsigned long long)w.cap ? (long)found : w.cap;
  for (long i = (long)blockIdx.x * 64 + threadIdx.x; i < n; i += (long)gridDim.x * 64) {
    const long* m = meta + (long)w.cand_file[i] * META;
    const long begin = m[0], size = m[1] - m[0], rel = w.cand_off[i] - begin;
    const FlacInfo si = load_info(m);
    FlacFrame fr;
    long end = 0;
    int st = flac_parse_header(bytes + begin, size, rel, si, &fr);
    if (st == NPPC_FLAC_OK) st = flac_decode_frame<false>(bytes + begin, size, rel, si, fr, 1, nullptr, nullptr, &end);
    w.cand_res[i] = st;
    w.cand_end[i] = end;
  }
}

// ---------------------------------------------------------------------------------------------------------------- chain
__global__ __launch_bounds__(64) void flac_chain_kernel(const unsigned char* __restrict__ bytes, const long* __restrict__ meta,
                                                        int nfiles, Work w, int* __restrict__ status) {
  const bool overflow = *w.counter > (unsigned long long)w.cap;
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f == 0) status[nfiles] = overflow;
  if (f >= nfiles) return;
  const long* m = meta + (long)f * META;
  const long begin = m[0], size = m[1] - m[0];
  const FlacInfo si = load_info(m);
  long off = si.first_frame, count = 0;
  int st = NPPC_FLAC_OK;
  while (count < si.total && !overflow) {                        // flac_decode_serial with the decode looked up
    FlacFrame fr;
    st = flac_parse_header(bytes + begin, size, off, si, &fr);
    if (st) break;
    if (fr.pos != count || fr.bs > si.total - count) {
      st = NPPC_FLAC_COUNT_MISMATCH;
      break;
    }
    const int idx = hash_find(w, begin + off);
    if (idx < 0 || idx >= w.cap) {                               // cannot be: every valid header below cap is in the table
      st = NPPC_FLAC_BAD_HEADER;
      break;
    }
    st = w.cand_res[idx];
    if (st) break;
    w.accepted[idx] = 1;
    count += fr.bs;
    off = w.cand_end[idx];                                       // > off: the parse read at least the header and a CRC-16
  }
  status[f] = st;
}

// --------------------------------------------------------------------------------------------------------------- decode
__global__ __launch_bounds__(64) void flac_decode_kernel(const unsigned char* __restrict__ bytes, const long* __restrict__ meta,
                                                         Work w, int* __restrict__ pcm, long pcm_elems,
                                                         float* __restrict__ mono, long mono_elems) {
  const unsigned long long found = *w.counter;
  const long n = found < (unsigned long long)w.cap ? (long)found : w.cap;
  for (long i = (long)blockIdx.x * 64 + threadIdx.x; i < n; i += (long)gridDim.x * 64) {
    if (!w.accepted[i]) continue;
    const long* m = meta + (long)w.cand_file[i] * META;
    const long begin = m[0], size = m[1] - m[0], rel = w.cand_off[i] - begin;
    const FlacInfo si = load_info(m);
    const long po = m[9], mo = m[10];
    if (po < 0 || si.total <= 0 || si.channels < 1 || si.channels > 8 || po > pcm_elems - si.channels * si.total) continue;
    const bool want_mono = mono != nullptr;
    if (want_mono && (mo < 0 || mo > mono_elems - si.total)) continue;
    FlacFrame fr;
    long end = 0;
    if (flac_parse_header(bytes + begin, size, rel, si, &fr) != NPPC_FLAC_OK) continue;
    flac_decode_frame<true>(bytes + begin, size, rel, si, fr, 0, pcm + po, want_mono ? mono + mo : nullptr, &end);
  }
}

int grid_for(long items, int per_block) {
  const long b = (items + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

}  // namespace

extern "C" {

int nppc_flac_probe(const unsigned char* bytes, long nbytes, long* info, int* status) {
  if (!bytes || !info || !status || nbytes < 0) return NPPC_EBADARG;
  if (nbytes >= (1L << 31)) return NPPC_EUNSUPPORTED;
  FlacInfo si = {};
  *status = flac_probe(bytes, nbytes, &si);
  info[0] = si.rate, info[1] = si.channels, info[2] = si.bps, info[3] = si.total, info[4] = si.min_bs, info[5] = si.max_bs;
  info[6] = si.first_frame, info[7] = 0;
  return NPPC_OK;
}

int nppc_flac_decode_host(const unsigned char* bytes, long nbytes, int* pcm, long pcm_elems, float* mono, long mono_elems,
                          int* status) {
  if (!bytes || !pcm || !status || nbytes < 0) return NPPC_EBADARG;
  if (nbytes >= (1L << 31)) return NPPC_EUNSUPPORTED;
  FlacInfo si = {};
  *status = flac_probe(bytes, nbytes, &si);
  if (*status) return NPPC_OK;
  if (pcm_elems < si.channels * si.total || (mono && mono_elems < si.total)) return NPPC_EBADARG;
  *status = flac_decode_serial(bytes, nbytes, si, pcm, mono);
  return NPPC_OK;
}

int nppc_flac_work_elems(long cap, long* elems) {
  if (!elems || cap < 1 || cap >= (1L << 31)) return NPPC_EBADARG;
  *elems = work_longs(cap);
  return NPPC_OK;
}

int nppc_flac_scan(const unsigned char* bytes, long total_bytes, const long* meta, int nfiles, long* work, long cap,
                   void* stream) {
  if (!bytes || !meta || !work || total_bytes <= 0 || nfiles <= 0 || cap < 1 || cap >= (1L << 31)) return NPPC_EBADARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(work, 0, (size_t)work_longs(cap) * sizeof(long), s) != hipSuccess) return NPPC_ELAUNCH;
  const int aligned = (reinterpret_cast<uintptr_t>(bytes) & 15) == 0;
  hipLaunchKernelGGL(flac_scan_kernel, dim3(grid_for((total_bytes + 15) >> 4, 256)), dim3(256), 0, s, bytes, total_bytes, meta,
                     nfiles, carve(work, cap), aligned);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_flac_parse(const unsigned char* bytes, const long* meta, int nfiles, long* work, long cap, void* stream) {
  if (!bytes || !meta || !work || nfiles <= 0 || cap < 1 || cap >= (1L << 31)) return NPPC_EBADARG;
  hipLaunchKernelGGL(flac_parse_kernel, dim3(grid_for(cap, 64)), dim3(64), 0, (hipStream_t)stream, bytes, meta, carve(work, cap));
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_flac_chain(const unsigned char* bytes, const long* meta, int nfiles, long* work, long cap, int* status, void* stream) {
  if (!bytes || !meta || !work || !status || nfiles <= 0 || cap < 1 || cap >= (1L << 31)) return NPPC_EBADARG;
  hipLaunchKernelGGL(flac_chain_kernel, dim3((nfiles + 63) / 64), dim3(64), 0, (hipStream_t)stream, bytes, meta, nfiles,
                     carve(work, cap), status);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

int nppc_flac_decode(const unsigned char* bytes, const long* meta, int nfiles, long* work, long cap, int* pcm, long pcm_elems,
                     float* mono, long mono_elems, void* stream) {
  if (!bytes || !meta || !work || !pcm || nfiles <= 0 || cap < 1 || cap >= (1L << 31) || pcm_elems <= 0 ||
      (mono && mono_elems <= 0))
    return NPPC_EBADARG;
  hipLaunchKernelGGL(flac_decode_kernel, dim3(grid_for(cap, 64)), dim3(64), 0, (hipStream_t)stream, bytes, meta, carve(work, cap),
                     pcm, pcm_elems, mono, mono_elems);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
