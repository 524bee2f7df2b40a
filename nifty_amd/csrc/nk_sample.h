// nk_sample.h -- per-element bodies of LinearInterpolator and RegriddingOperator (nifty_amd/sampling_operators.py,
// docs/SAMPLING.md; reference operators/linear_interpolation.py, operators/regridding_operator.py).
//
// Multilinear interpolation on a periodic grid of 1-3 axes: a point with base cell c (grid index per axis) and fractions
// e_a in [0, 1) reads the 2^d corners (c_a + m_a) mod n_a, m in {0, 1}^d in C order (axis 0 slowest), with the weights
// prod_a (m_a ? e_a : 1 - e_a), the product taken in axis order.  The reference writes that matrix down (scipy coo); here
// the weights are formed in registers from e, so the plan holds 8 d + 24 bytes per point instead of 2 x 2^d x 8.
// Regridding along one axis of an (outer, n, inner) view: new[j] = old[b_j] (1 - f_j) + old[b_j + 1] f_j.
// Every product and sum is fp64 and rounds separately (NK_NO_CONTRACT): the host path of the operators (numpy) and the
// test-only emulation (tests/emu/emu_sample.cpp) run the same operations in the same order.
#pragma once
#include <stdint.h>

#include "nk_core.h"

#if defined(__clang__)
#define NK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NK_NO_CONTRACT
#endif

#define NK_SAMPLE_BLOCK 256  // threads of every launch; one workgroup sums one LONG cell of the adjoint
#define NK_SAMPLE_LONG 128   // an occupied cell with more points than this is LONG (the plan lists those cells)

// grid index per axis of a flat cell index (any 64-bit pattern decodes to indices inside the grid)
template <int ND>
NK_HD void nk_sample_decode(int64_t cell, const int64_t* n, int64_t* idx) {
  uint64_t r = (uint64_t)cell;
  for (int a = ND - 1; a >= 0; --a) {
    if (r <= 0xffffffffull && n[a] <= 0xffffffffll) {  // (64-bit division is a long software routine on the device)
      const uint32_t r32 = (uint32_t)r, na = (uint32_t)n[a];
      idx[a] = (int64_t)(r32 % na);
      r = r32 / na;
    } else {
      idx[a] = (int64_t)(r % (uint64_t)n[a]);
      r /= (uint64_t)n[a];
    }
  }
}

// weight of corner m (bit of axis a = (m >> (ND - 1 - a)) & 1) from the point's fractions
template <int ND>
NK_HD double nk_sample_weight(const double* e, int m) {
  NK_NO_CONTRACT
  double w = 0.0;
  for (int a = 0; a < ND; ++a) {
    const double f = ((m >> (ND - 1 - a)) & 1) ? e[a] : 1.0 - e[a];
    w = a == 0 ? f : w * f;
  }
  return w;
}

// flat index of corner m of the cell idx[], wrapped
template <int ND>
NK_HD int64_t nk_sample_corner(const int64_t* idx, const int64_t* n, int m) {
  int64_t flat = 0;
  for (int a = 0; a < ND; ++a) {
    int64_t i = idx[a] + ((m >> (ND - 1 - a)) & 1);
    i -= i >= n[a] ? n[a] : 0;
    flat = flat * n[a] + i;
  }
  return flat;
}

// TIMES of one point: sum_m w_m x[corner_m], the 2^d products added in corner order
template <typename T, int ND>
NK_HD double nk_sample_gather(const int64_t* n, int64_t cell, const double* e, const T* x) {
  NK_NO_CONTRACT
  int64_t idx[ND];
  nk_sample_decode<ND>(cell, n, idx);
  double acc = 0.0;
  for (int m = 0; m < (1 << ND); ++m) acc += nk_sample_weight<ND>(e, m) * (double)x[nk_sample_corner<ND>(idx, n, m)];
  return acc;
}

// ADJOINT_TIMES, corner m of one occupied cell: the sorted points lo, lo + stride, ... < hi of the cell's list, in that
// order.  y is in the caller's order (perm[k] = original index of sorted point k).
template <typename T, int ND>
NK_HD double nk_sample_cell_sum(const double* frac, const int64_t* perm, const T* y, int64_t npoints, int m, int64_t lo,
                                int64_t hi, int64_t stride) {
  NK_NO_CONTRACT
  double acc = 0.0;
  for (int64_t k = lo; k < hi; k += stride) {
    const int64_t o = perm[k];
    if ((uint64_t)o < (uint64_t)npoints) acc += nk_sample_weight<ND>(frac + k * ND, m) * (double)y[o];
  }
  return acc;
}

// The points of a LONG cell are dealt to the NK_SAMPLE_BLOCK threads of one workgroup round-robin (thread t sums the list
// positions t, t + 256, ... with nk_sample_cell_sum), and the 256 partial sums are joined by a fixed tree: a xor butterfly
// over the 64 lanes of each wavefront (offsets 32, 16, .. 1), then the four wavefronts in order.  The device does the
// butterfly with __shfl_xor (nk_sample.hip); this is the same tree on an array, for the host emulation.
#ifdef NK_HOST_EMU
inline double nk_sample_tree_host(double* p) {
  for (int w = 0; w < NK_SAMPLE_BLOCK / 64; ++w) {
    double* q = p + 64 * w;
    for (int off = 32; off > 0; off >>= 1) {
      double nxt[64];
      for (int l = 0; l < 64; ++l) nxt[l] = q[l] + q[l ^ off];
      for (int l = 0; l < 64; ++l) q[l] = nxt[l];
    }
  }
  double total = p[0];
  for (int w = 1; w < NK_SAMPLE_BLOCK / 64; ++w) total += p[64 * w];
  return total;
}
#endif

// RegriddingOperator TIMES along one axis: col points at old index 0 of the output's (outer, inner) column
template <typename TI>
NK_HD double nk_regrid_gather(const TI* col, int64_t stride, int64_t b, double f) {
  NK_NO_CONTRACT
  const double lo = (double)col[b * stride] * (1.0 - f);
  return lo + (double)col[(b + 1) * stride] * f;
}

// RegriddingOperator ADJOINT_TIMES along one axis, old cell i: rstart[i] = first new index j with b_j >= i (b is
// non-decreasing), so b_j = i on [rstart[i], rstart[i + 1]) -- weight 1 - f_j -- and b_j = i - 1 on [rstart[i - 1],
// rstart[i]) -- weight f_j; ascending j, first range first (the order of the reference's two add_at calls)
template <typename TI>
NK_HD double nk_regrid_scatter(const TI* col, int64_t stride, const int64_t* rstart, const double* frac, int64_t i,
                               int64_t n_new) {
  NK_NO_CONTRACT
  double acc = 0.0;
  int64_t j0 = rstart[i], j1 = rstart[i + 1];
  j0 = j0 < 0 ? 0 : j0;
  j1 = j1 > n_new ? n_new : j1;
  for (int64_t j = j0; j < j1; ++j) acc += (double)col[j * stride] * (1.0 - frac[j]);
  if (i > 0) {
    int64_t k0 = rstart[i - 1];
    k0 = k0 < 0 ? 0 : k0;
    const int64_t k1 = j0 > n_new ? n_new : j0;
    for (int64_t j = k0; j < k1; ++j) acc += (double)col[j * stride] * frac[j];
  }
  return acc;
}
