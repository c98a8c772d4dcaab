// Cyclic Jacobi eigen-solver of the per-item K x K Gram matrices of the MC-dropout PCA: shared by the uniform path
// (mc_pca.hip) and the ragged-gap path (mc_pca_ragged.hip).  One workgroup per item, fp64 in LDS, no atomics: the
// result is a function of the item's Gram alone.
#pragma once
#include "common.h"

namespace {

constexpr int PCA_KMAX = 60;

// cyclic Jacobi on the symmetric K x K Gram of one item (fp64, LDS); round-robin pairing -> K/2 disjoint rotations per
// round.  Writes the n largest eigenvalues (descending) and their eigenvectors evec[b][i][k].
__global__ __launch_bounds__(256) void pca_eigh_kernel(const double* __restrict__ G, double* __restrict__ eval,
                                                       double* __restrict__ evec, int K, int n) {
  __shared__ double A[PCA_KMAX][PCA_KMAX];
  __shared__ double V[PCA_KMAX][PCA_KMAX];
  __shared__ double cs[PCA_KMAX / 2][2];
  __shared__ int pq[PCA_KMAX / 2][2];
  __shared__ double red[4], red2[4];
  __shared__ int order[PCA_KMAX];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Kp = (K + 1) & ~1, half = Kp / 2;                  // odd K: one padding row/column of zeros (eigenvalue 0)
  for (int e = tid; e < Kp * Kp; e += 256) {
    const int i = e / Kp, j = e % Kp;
    A[i][j] = (i < K && j < K) ? G[((size_t)b * K + i) * K + j] : 0.0;
    V[i][j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int e = tid; e < Kp * Kp; e += 256) {
      const int i = e / Kp, j = e % Kp;
      const double a = A[i][j];
      if (i == j) dg += a * a; else off += a * a;
    }
    off = wave_sum(off);
    dg = wave_sum(dg);
    __syncthreads();
    if (lane == 0) { red[wave] = off; red2[wave] = dg; }
    __syncthreads();
    const double offt = red[0] + red[1] + red[2] + red[3], dgt = red2[0] + red2[1] + red2[2] + red2[3];
    __syncthreads();
    if (offt <= 1e-30 * dgt || offt == 0.0) break;
    for (int r = 0; r < Kp - 1; ++r) {
      if (tid < half) {
        int p, q;
        if (tid == 0) { p = Kp - 1; q = r; }
        else { p = (r + tid) % (Kp - 1); q = (r - tid + Kp - 1) % (Kp - 1); }
        if (p > q) { const int t = p; p = q; q = t; }
        const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
        double c = 1.0, s = 0.0;
        if (fabs(apq) > 1e-300 && fabs(apq) > 1e-17 * sqrt(fabs(app * aqq)) ) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        pq[tid][0] = p; pq[tid][1] = q;
        cs[tid][0] = c; cs[tid][1] = s;
      }
      __syncthreads();
      for (int e = tid; e < half * Kp; e += 256) {               // columns p, q of A and V
        const int m = e / Kp, k = e % Kp, p = pq[m][0], q = pq[m][1];
        const double c = cs[m][0], s = cs[m][1];
        const double ap = A[k][p], aq = A[k][q];
        A[k][p] = c * ap - s * aq;
        A[k][q] = s * ap + c * aq;
        const double vp = V[k][p], vq = V[k][q];
        V[k][p] = c * vp - s * vq;
        V[k][q] = s * vp + c * vq;
      }
      __syncthreads();
      for (int e = tid; e < half * Kp; e += 256) {               // rows p, q of A
        const int m = e / Kp, k = e % Kp, p = pq[m][0], q = pq[m][1];
        const double c = cs[m][0], s = cs[m][1];
        const double ap = A[p][k], aq = A[q][k];
        A[p][k] = c * ap - s * aq;
        A[q][k] = s * ap + c * aq;
      }
      __syncthreads();
    }
  }
  if (tid == 0) {                                               // selection of the n largest (K <= 60, n <= 8)
    for (int i = 0; i < Kp; ++i) order[i] = i;
    for (int i = 0; i < n; ++i) {
      int best = i;
      for (int j = i + 1; j < Kp; ++j)
        if (A[order[j]][order[j]] > A[order[best]][order[best]]) best = j;
      const int t = order[i]; order[i] = order[best]; order[best] = t;
    }
  }
  __syncthreads();
  for (int e = tid; e < n * K; e += 256) {
    const int i = e / K, k = e % K;
    evec[((size_t)b * n + i) * K + k] = V[k][order[i]];
  }
  if (tid < n) eval[(size_t)b * n + tid] = A[order[tid]][order[tid]];
}

}  // namespace
