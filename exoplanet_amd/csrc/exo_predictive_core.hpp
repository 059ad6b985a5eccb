// exo_predictive_core.hpp -- the per-column arithmetic of the posterior bands (exoplanet_amd/predictive.py, quantiles / bands;
// exo_column_quantiles_f64): order statistics of the non-NaN values of one column of an (S, N) array, along the strided axis,
// and the linear interpolation between two of them at a position formed from whole numbers.  Definition: DESIGN.md section 24.
// Compiles for the device (exo_predictive.hip) and, with EXO_HOST_BUILD, for the host (tests/predictive_harness.cpp checks it
// against the numpy restatement tests/predictive_oracle.py without a GPU).
//
// The selection is that of exo_detrend_core.hpp (double_key; select_kth: the k-th smallest is the largest key x with
// #{v < x} <= k, found by counting passes that compare doubles; select_next: one more pass), restated for this geometry: a
// column is read by many lanes, each a share of its rows, so a pass is split into what a lane accumulates (integers and
// keys), an exact merge of those, and a decision every lane of the column repeats.  Two things differ from select_kth.  All Q
// order statistics of a column are searched in the SAME pass, and the search is on the interval [key of the minimum, key of
// the maximum] found by the first pass instead of on 64 bits -- which is what the shared sign, exponent and leading mantissa
// bits of a column's values buy -- with K = 2^B - 1 trial values per order statistic and pass (Q K counters): the interval
// shrinks by B bits per pass, ceil(ceil(log2(number of keys in the interval)) / B) passes.  A pass is bound by the memory it
// streams, not by its comparisons, so B > 1 is all gain for as long as the Q K trial values and counters fit in registers.
// Nothing here sorts or stores.
#pragma once
#include <math.h>
#include <stdint.h>

#include "exo_detrend_core.hpp"

#define EXO_PRED_HD EXO_DET_HD

namespace predictive {

using detrend::double_key;
using detrend::key_double;

constexpr int kMaxQ = 16;  // EXO_QUANTILE_MAX_Q

// the strided column accessor: row i of one column of a row-major array whose rows are `stride` doubles apart
struct Column {
  const double* p;
  int64_t stride;
  EXO_PRED_HD double operator[](int64_t i) const { return p[i * stride]; }
};

// ---- the whole-number rank rule ------------------------------------------------------------------------------------------------
// percent / 100 = a / b exactly; among m >= 1 values the position is (m - 1) a / b = lo + rem / b.  (m < 2^31, a <= b <= 1e9:
// the product stays below 2^61.)
struct Rank {
  int32_t lo, rem;   // (lo <= m - 1 < 2^31, rem < b <= 1e9)
};

EXO_PRED_HD Rank rank_of(int64_t m, int64_t a, int64_t b) {
  const int64_t num = (m - 1) * a;
  return Rank{(int32_t)(num / b), (int32_t)(num % b)};
}

// x_(lo) + (rem / b) (x_(lo+1) - x_(lo)): one division, one subtraction, one multiplication, one addition (compiled without
// contraction into a fused multiply-add).  rem == 0: x_(lo) itself, no arithmetic.
EXO_PRED_HD double interpolate(double x0, double x1, int32_t rem, int64_t b) {
  if (rem == 0) return x0;
  const double frac = (double)rem / (double)b;
  const double d = x1 - x0;
  const double s = frac * d;
  return x0 + s;
}

// ---- first pass: how many values take part, and between which keys they lie ------------------------------------------------------
// Keys are those of v + 0.0, so that a zero of either sign has the key of +0: the selection below compares doubles, for which
// the two are one number, and +0 is the key it arrives at (select_kth: "a zero comes back as +0").
struct Extent {
  int32_t m;
  uint64_t kmin, kmax;
};

EXO_PRED_HD Extent extent_empty() { return Extent{0, ~0ull, 0ull}; }

EXO_PRED_HD void extent_add(Extent& e, double v) {
  const bool in = v == v;
  const uint64_t k = double_key(v + 0.0);
  e.m += in ? 1 : 0;
  e.kmin = (in && k < e.kmin) ? k : e.kmin;
  e.kmax = (in && k > e.kmax) ? k : e.kmax;
}

// (integers: exact in any order)
EXO_PRED_HD void extent_merge(Extent& e, int32_t m, uint64_t kmin, uint64_t kmax) {
  e.m += m;
  e.kmin = kmin < e.kmin ? kmin : e.kmin;
  e.kmax = kmax > e.kmax ? kmax : e.kmax;
}

// bits of the interval of kmax - kmin + 1 keys: ceil(log2(kmax - kmin + 1)); none for an empty or a constant column.  A
// search that settles B bits per pass takes ceil(bits / B) passes.
EXO_PRED_HD int interval_bits(const Extent& e) {
  if (e.m == 0 || e.kmax <= e.kmin) return 0;
  uint64_t span = e.kmax - e.kmin;  // >= 1
  int bits = 0;
  while (span) {
    ++bits;
    span >>= 1;
  }
  return bits;
}

EXO_PRED_HD int passes_needed(const Extent& e, int B) { return (interval_bits(e) + B - 1) / B; }

// ---- the search for Q order statistics at once -----------------------------------------------------------------------------------
// For each q the key of x_(k[q]) is the largest key x with #{v < x} <= k[q]; it lies in [lo[q], hi[q]], and
// #{v < key_double(lo[q])} <= k[q] throughout.  A pass counts c_j = #{v < trial j} for the K trial keys t_1 <= ... <= t_K of
// every q, which cut the interval into K + 1 runs of at most ceil(keys / (K + 1)) keys; the counts are monotone in j, so the
// number of them that are <= k names the run that holds the answer.  Trials past the end of a short interval repeat hi (equal
// trials, equal counts: harmless), and an interval that is down to one key stays as it is, so a column that needs fewer
// passes than its neighbours takes the extra ones unharmed.  Every key of [kmin, kmax] is that of a number: no trial is a NaN.
template <int Q>
struct Bisect {
  uint64_t lo[Q], hi[Q];
  int32_t k[Q];
};

template <int Q>
EXO_PRED_HD void bisect_begin(Bisect<Q>& s, const Extent& e, const Rank* rank) {
  for (int q = 0; q < Q; ++q) {
    s.lo[q] = e.m ? e.kmin : 0;
    s.hi[q] = e.m ? e.kmax : 0;
    s.k[q] = rank[q].lo;
  }
}

// trial key j = 1 .. K of order statistic q (j = 0: lo itself)
template <int K, int Q>
EXO_PRED_HD uint64_t bisect_key(const Bisect<Q>& s, int q, int j) {
  const uint64_t n = s.hi[q] - s.lo[q];        // keys - 1
  const uint64_t run = n / (K + 1) + 1;        // ceil(keys / (K + 1))          (K <= 7: j run stays below 2^64)
  const uint64_t off = (uint64_t)j * run;
  return off > n ? s.hi[q] : s.lo[q] + off;
}

template <int K, int Q>
EXO_PRED_HD double bisect_trial(const Bisect<Q>& s, int q, int j) { return key_double(bisect_key<K>(s, q, j)); }

// count[j - 1] = #{v < trial j}, j = 1 .. K
template <int K, int Q>
EXO_PRED_HD void bisect_decide(Bisect<Q>& s, int q, const int32_t* count) {
  int below = 0;
  for (int j = 0; j < K; ++j) below += (count[j] <= s.k[q]) ? 1 : 0;
  const uint64_t lo = below ? bisect_key<K>(s, q, below) : s.lo[q];
  const uint64_t hi = below < K ? bisect_key<K>(s, q, below + 1) - 1 : s.hi[q];   // (count > k there: that trial lies above lo)
  s.lo[q] = lo;
  s.hi[q] = hi;
}

template <int Q>
EXO_PRED_HD double bisect_value(const Bisect<Q>& s, int q) { return key_double(s.lo[q]) + 0.0; }

// ---- the value after x_(k) in the sorted order (select_next, Q at once) ---------------------------------------------------------
// c = #{v <= a}, up = the smallest value above a; x_(k+1) is a where c >= k + 2 (a tie), else up
struct Next {
  int32_t c;
  double up;
};

EXO_PRED_HD void next_add(Next& s, double v, double a) {
  s.c += (v <= a) ? 1 : 0;
  s.up = (v > a && v < s.up) ? v : s.up;
}

// (a count and a minimum: exact in any order)
EXO_PRED_HD void next_merge(Next& s, int32_t c, double up) {
  s.c += c;
  s.up = up < s.up ? up : s.up;
}

EXO_PRED_HD double next_value(const Next& s, int32_t k, double a) { return s.c >= k + 2 ? a : s.up; }

// ---- the per-column routine ------------------------------------------------------------------------------------------------------
// Q quantiles (num[q] / den[q], 0 <= num <= den) of the non-NaN values among col[0 .. n_rows - 1]: out[q * out_stride].  Returns
// the number of values that took part; none: NaN everywhere.  B: the bits a pass settles (2^B - 1 trial values per quantile).  *n_pass, when given: the passes over the column.  This is one
// lane owning the whole column; the kernel runs the same steps with the rows shared out and a merge after each pass.
template <int Q, int B, class P>
EXO_PRED_HD int32_t column_quantiles(P col, int64_t n_rows, const int64_t* num, const int64_t* den, double* out, int64_t out_stride,
                                     int* n_pass) {
  Extent e = extent_empty();
  for (int64_t i = 0; i < n_rows; ++i) extent_add(e, col[i]);
  int passes = 1;
  if (e.m == 0) {
    for (int q = 0; q < Q; ++q) out[q * out_stride] = NAN;
    if (n_pass) *n_pass = passes;
    return 0;
  }
  Rank rank[Q];
  bool two = false;
  for (int q = 0; q < Q; ++q) {
    rank[q] = rank_of(e.m, num[q], den[q]);
    two = two || rank[q].rem != 0;
  }
  Bisect<Q> s;
  bisect_begin<Q>(s, e, rank);
  constexpr int K = (1 << B) - 1;
  const int need = passes_needed(e, B);
  for (int pass = 0; pass < need; ++pass) {
    double x[Q * K];
    int32_t c[Q * K];
    for (int q = 0; q < Q; ++q)
      for (int j = 0; j < K; ++j) {
        x[q * K + j] = bisect_trial<K>(s, q, j + 1);
        c[q * K + j] = 0;
      }
    for (int64_t i = 0; i < n_rows; ++i) {
      const double v = col[i];
      for (int u = 0; u < Q * K; ++u) c[u] += (v < x[u]) ? 1 : 0;
    }
    for (int q = 0; q < Q; ++q) bisect_decide<K>(s, q, c + q * K);
  }
  passes += need;
  double a[Q];
  Next nx[Q];
  for (int q = 0; q < Q; ++q) {
    a[q] = bisect_value<Q>(s, q);
    nx[q] = Next{0, INFINITY};
  }
  if (two) {
    for (int64_t i = 0; i < n_rows; ++i) {
      const double v = col[i];
      for (int q = 0; q < Q; ++q) next_add(nx[q], v, a[q]);
    }
    ++passes;
  }
  for (int q = 0; q < Q; ++q)
    out[q * out_stride] = interpolate(a[q], rank[q].rem ? next_value(nx[q], s.k[q], a[q]) : a[q], rank[q].rem, den[q]);
  if (n_pass) *n_pass = passes;
  return e.m;
}

}  // namespace predictive
