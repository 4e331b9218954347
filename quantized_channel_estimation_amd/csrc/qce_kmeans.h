// Lloyd's k-means on the device (qce_kmeans.hip): the plan and the launchers qce_capi_kmeans.hip drives.
// Data: X (B, D = 2N) doubles, the interleaved real view of the complex rows; a column mean is subtracted as rows are
// loaded.  Centres live in padded (KP, DP) buffers (KP, DP = K, D rounded up to 16, pads zero) so the MFMA loops carry
// no bounds tests on them.
#pragma once
#include <hip/hip_runtime.h>

struct QceKmPlan {
  long long B = 0;
  int D = 0, K = 0;
  int DP = 0, KP = 0;   // D, K rounded up to 16
  int W = 0;            // 16-row tiles (and waves) per assignment workgroup
  int nwg = 0;          // assignment workgroups
  long long chunk = 0;  // rows per accumulation chunk (a multiple of 16)
  int C = 0;            // accumulation chunks
  int nct = 0;          // column jobs per cluster block (4 column tiles of 16 each)
};
QceKmPlan qce_km_plan(long long B, int N, int K);

// cnorm (KP): |c_k|^2, +inf for the pad clusters
hipError_t qce_launch_km_cnorm(const QceKmPlan& p, const double* C, double* cnorm, hipStream_t st);
// labels (B) int64 in/out (the previous labels are read for the changed count); pchanged (nwg)
hipError_t qce_launch_km_assign(const QceKmPlan& p, const double* X, const double* mean, const double* C,
                                const double* cnorm, long long* labels, int* pchanged, hipStream_t st);
// part (C, KP, DP), pcount (C, KP): per-chunk sums and counts
hipError_t qce_launch_km_accum(const QceKmPlan& p, const double* X, const double* mean, const long long* labels,
                               double* part, double* pcount, hipStream_t st);
// sums (KP, DP), counts (KP): the partials added in a fixed order
hipError_t qce_launch_km_sums(const QceKmPlan& p, const double* part, const double* pcount, double* sums,
                              double* counts, hipStream_t st);
// Cnew = sums / counts; status = {sum (Cnew - Ccur)^2, changed labels, empty clusters}
hipError_t qce_launch_km_finalize(const QceKmPlan& p, const double* sums, const double* counts, const int* pchanged,
                                  const double* Ccur, double* Cnew, double* status, hipStream_t st);
// rows far[0..e) leave their clusters' sums and become the sums of the clusters empt[0..e), in this order
hipError_t qce_launch_km_relocate(const QceKmPlan& p, const double* X, const double* mean, const long long* labels,
                                  const long long* far, const int* empt, int e, double* sums, double* counts,
                                  hipStream_t st);
// dist (B): |x_b - c_label(b)|^2 in the difference form
hipError_t qce_launch_km_rowdist(const QceKmPlan& p, const double* X, const double* mean, const double* C,
                                 const long long* labels, double* dist, hipStream_t st);
// out[0] = sum of v[0..n) in a fixed order
hipError_t qce_launch_km_vsum(long long n, const double* v, double* out, hipStream_t st);
// resp (B, K): 1.0 at the label, 0.0 elsewhere
hipError_t qce_launch_km_onehot(const QceKmPlan& p, const long long* labels, double* resp, hipStream_t st);

// k-means++ seeding from pre-drawn uniforms (qce_kmeans_seed.hip).  closest[b] lives in a row of a (T, stride) scratch
// buffer, stride = C * chunk >= B (rows past B hold zeros), with (T, C) per-chunk partial sums beside it.
struct QceKmSeedPlan {
  long long B = 0;
  int N = 0, NP = 0;     // complex elements per row, rounded up to 64
  long long chunk = 0;   // rows per chunk (a multiple of 64), one candidate-pass workgroup each
  int C = 0;             // chunks (<= 1024)
  long long stride = 0;  // C * chunk
};
QceKmSeedPlan qce_km_seed_plan(long long B, int N);
// out (T, stride), part (T, C): min(closest, |x_b - x_cand[t]|^2) and its chunk sums, 1 <= T <= 16; closest = row
// win[0] of the scratch buffer `closest` (NULL: +inf, the pass of the first centre, `win` unused)
hipError_t qce_launch_km_seed_cand(const QceKmSeedPlan& p, int T, const double* X, const double* mean,
                                   const long long* cand, const double* closest, const int* win, double* out,
                                   double* part, hipStream_t st);
// From the last pass (part, scratch, cand_prev; Tprev rows): idx_out[0], pot_out[0], win_out[0] = the candidate with
// the first smallest potential, that potential and its scratch row; cand_next[t] = the first row whose inclusive
// cumulative sum of that scratch row is >= u[t] * pot, clipped to B - 1, for t < Tn (Tn = 0: no search)
hipError_t qce_launch_km_seed_pick(const QceKmSeedPlan& p, int Tprev, const double* part, const double* scratch,
                                   const long long* cand_prev, const double* u, int Tn, long long* idx_out,
                                   double* pot_out, int* win_out, long long* cand_next, hipStream_t st);
// centers (K, 2N) = X[idx[k]] - mean
hipError_t qce_launch_km_seed_gather(const QceKmSeedPlan& p, int K, const double* X, const double* mean,
                                     const long long* idx, double* centers, hipStream_t st);
