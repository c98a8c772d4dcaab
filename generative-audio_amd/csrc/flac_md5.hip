// MD5 of decoded FLAC samples for gfx950 (nppc_audio/flac.py).  The hash itself is csrc/md5_core.h,
// shared with the host entry points below and with tools/check/md5_host_check.cc.
//   nppc_flac_stream_md5   host only: the 16 bytes STREAMINFO holds
//   nppc_flac_md5_host     host only: the serial hash of one [C][n] block of samples
//   nppc_flac_md5          one lane per file: its whole chain of blocks, then the comparison with the stated digest
// MD5 is a serial chain over a file's blocks, so the parallelism is across files.  Lane i takes file order[i]; with the
// files ordered by descending message length the lanes of a wave run similar block counts.  Workgroups are one wave.  No
// barrier, no LDS, no atomic: a lane reads its file's samples and writes digest[f][0..16) and verdict[f], nothing else, so
// no result depends on `order`, on the neighbours or on the run.  Lanes of one wave whose files take different formers
// (16-bit mono, 16-bit stereo, the general one) run them one after the other.
#include "common.h"
#include "flac_core.h"
#include "md5_core.h"
#include "nppc_hip.h"

namespace {

constexpr int META = NPPC_FLAC_META;

__global__ __launch_bounds__(64) void flac_md5_kernel(const int* __restrict__ pcm, long pcm_elems, const long* __restrict__ meta,
                                                      int nfiles, const int* __restrict__ order,
                                                      const unsigned char* __restrict__ expected, const int* __restrict__ status,
                                                      unsigned char* __restrict__ digest, int* __restrict__ verdict) {
  const int lane = blockIdx.x * 64 + threadIdx.x;
  if (lane >= nfiles) return;
  const int f = order[lane];
  if (f < 0 || f >= nfiles) return;                              // not a file of this batch: nothing to write to
  const long* m = meta + (long)f * META;
  const long channels = m[3], bps = m[4], total = m[7], po = m[9];
  unsigned char* out = digest + (long)f * 16;
  // total < 2^36 (STREAMINFO's field) keeps channels * total inside int64
  const bool skip = (status && status[f] != 0) || channels < 1 || channels > 8 || bps < 4 || bps > 32 || total < 0 ||
                    total >= (1L << 36) || po < 0 || po > pcm_elems - channels * total;
  if (skip) {
    for (int i = 0; i < 16; ++i) out[i] = 0;
    verdict[f] = 0;
    return;
  }
  unsigned char d[16];
  md5_pcm(pcm + po, total, (int)channels, (int)bps, d);
  int v = 0;
  if (expected) {
    const unsigned char* e = expected + (long)f * 16;
    unsigned any = 0, diff = 0;
    for (int i = 0; i < 16; ++i) any |= e[i], diff |= (unsigned)(e[i] ^ d[i]);
    v = !any ? 0 : diff ? 2 : 1;                                 // sixteen zero bytes: the format's "not computed"
  }
  for (int i = 0; i < 16; ++i) out[i] = d[i];
  verdict[f] = v;
}

}  // namespace

extern "C" {

int nppc_flac_stream_md5(const unsigned char* bytes, long nbytes, unsigned char* md5, int* present, int* status) {
  if (!bytes || !md5 || !present || !status || nbytes < 0) return NPPC_EBADARG;
  if (nbytes >= (1L << 31)) return NPPC_EUNSUPPORTED;
  FlacInfo si = {};
  *status = flac_probe(bytes, nbytes, &si);
  *present = 0;
  for (int i = 0; i < 16; ++i) md5[i] = 0;
  if (*status) return NPPC_OK;
  // flac_probe accepted a 34-byte STREAMINFO at byte 8: its MD5 field is bytes 26..42
  for (int i = 0; i < 16; ++i) md5[i] = bytes[26 + i], *present |= bytes[26 + i] != 0;
  return NPPC_OK;
}

int nppc_flac_md5_host(const int* pcm, long n, int channels, int bps, unsigned char* digest) {
  if (!digest || n < 0 || (!pcm && n > 0) || channels < 1 || channels > 8 || bps < 4 || bps > 32 || n >= (1L << 56))
    return NPPC_EBADARG;
  md5_pcm(pcm, n, channels, bps, digest);
  return NPPC_OK;
}

int nppc_flac_md5(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* order, const unsigned char* expected,
                  const int* status, unsigned char* digest, int* verdict, void* stream) {
  if (!meta || !order || !digest || !verdict || nfiles <= 0 || pcm_elems < 0 || (!pcm && pcm_elems > 0)) return NPPC_EBADARG;
  hipLaunchKernelGGL(flac_md5_kernel, dim3((nfiles + 63) / 64), dim3(64), 0, (hipStream_t)stream, pcm, pcm_elems, meta, nfiles,
                     order, expected, status, digest, verdict);
  NPPC_CHECK_LAUNCH();
  return NPPC_OK;
}

}  // extern "C"
