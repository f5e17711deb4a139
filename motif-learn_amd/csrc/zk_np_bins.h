// zk_np_bins.h -- the bin np.histogram(x, bins=256) counts a value in, one value at a time: the rule the histograms of
// estimate_d (zk_knn.hip, hist_kernel) and Otsu's threshold of com_refine (zk_com_refine.hip, otsu_threshold) share.
//
// Only units built with -ffp-contract=off include this header: the index is NumPy's (v - first) / (last - first) * 256 with every
// operation rounded once, and the edges it is corrected against are the caller's (np.linspace's values).
#pragma once

namespace {

constexpr int BINS = 256;

// edges: the BINS + 1 edges, edges[0] = first and edges[BINS] = last
__device__ inline int np_bin(double v, double first, double last, const double* edges) {
  const double f = ((v - first) / (last - first)) * (double)BINS;
  int b = f >= (double)BINS ? BINS - 1 : (f > 0 ? (int)f : 0);               // truncation; 256 folds into 255 (a NaN goes to 0)
  if (v < edges[b] && b > 0) --b;
  if (v >= edges[b + 1] && b != BINS - 1) ++b;
  return b;
}

}  // namespace
