// Random-SNR observations and the VAE encoder's input features in one pass (reference utils.py:254-318
// get_observation_nbit_randSNR*, estimators/vae.py:46-53 and :89-94):
//   i_b = supplied SNR index of row b, or a draw from {0..S-1} (cumulative probabilities cdf, or uniform)
//   v   = A h_b + scales[i_b] * w_b          w_b supplied, or drawn on the device
//   y_b = Q_{i_b}(v)                         1 bit / per-SNR tables thr[i_b], lab[i_b] / none
// and either y (B, M) complex128 is stored, or the encoder features (B, P, 2N) float32, M = P N: row (b, p) is
// [Re f | Im f] with f = y_b[pN:(p+1)N] ("raw") or its unitary DFT.  With features the complex128 y never
// reaches memory.
//
// Arithmetic: observe_one, and for a dense A cfma in column order, exactly as k_observe_id / k_observe_a
// (qce_observe.hip): the same bits as qce_observe row by row.  A = kron(x, I_N) (found on the host, entry for entry)
// keeps only the one structurally non-zero term of each row sum; every other term is a signed zero, which changes
// no finite sum.  That term is formed as numpy's matmul forms it, Re = rnd(rnd(xr hr) - rnd(xi hi)) and
// Im = rnd(rnd(xr hi) + rnd(xi hr)) (its BLAS kernels keep the real-real and imaginary-imaginary products in separate
// accumulators), so an unquantised y equals the reference's bit for bit as well.  cfma fuses the second product of each
// part into the sum and can differ from that in the last bit: on the fixture (tests/golden/randsnr.npz) the two
// routes give the same quantised y and unquantised values one rounding apart.
//
// Draws: Philox4x32-10 keyed by `seed`.  The noise of complex element (b, m) uses counter (row_offset + b) M + m in
// the noise domain of qce_observe.hip (S = 1 reproduces qce_observe with offset = row_offset M); the SNR index of
// row b uses counter row_offset + b in a domain of its own, u in [0, 1) from 53 bits, index = #{cdf[i] <= u}
// clamped to S - 1 (uniform: floor(u S)).  Any chunking of a batch by rows draws the same numbers.
//
// One workgroup (256 threads) walks tiles of G segments; a segment is one row of the output: N values of one (b, p)
// for features (G = 1024 / N), the M values of row b for y.  Per tile: the segments' SNR indices go to LDS, every
// thread then produces elements (16-byte coalesced loads of h and w).  y is stored at once; for features the
// quantised values stay in LDS (row stride N + 1), a radix-2 FP64 transform runs over all rows of the tile, and the
// float32 conversion happens at the store (16 bytes per lane, rows contiguous).  The noise scales, and the
// quantiser tables when S (2L - 1) doubles fit QCE_ROWS_TABLE_LDS (32 KiB: with the 17 KiB tile that keeps three
// workgroups on a CU's 160 KiB), are copied to LDS once per workgroup; larger tables (S = 64 at 8 bits is 256 KiB) are
// read from global memory, where the few that a tile touches stay in L2.
//
// Roofline: HBM.  Algorithmic bytes per complex element: features 16 (h) + 8 (float pair); y 16 + 16; + 16 with
// supplied noise.  A dense A adds its L2-resident read.  Measured with generated noise: 1.4 TB/s for
// features and 2.7 TB/s for y of the 8 TB/s peak, so the generator's FP64 arithmetic and the LDS transform, not the
// memory system, set the pace.
#include "qce_common.h"
#include "qce_kernels.h"
#include "qce_observe_dev.h"

namespace {

using namespace qce_obs;

constexpr int ROWS_THREADS = 256;
constexpr int FEAT_TILE = 1024;   // complex values per feature tile (G = FEAT_TILE / N rows)
constexpr int Y_TILE = 2048;      // target complex values per y tile
constexpr int MAX_SEGS = 256;     // rows per tile at most (FEAT_TILE / 16 = 64 for features)
constexpr int MAX_BLOCKS = 2048;  // 8 workgroups per CU; the tiles beyond are walked grid-stride (a grid sized
                                  // to the occupancy query measured no faster)

struct RowsPlan {
  int SL;    // segment length: N (features) or M (y)
  int lgSL;  // log2(SL) for features
  int SPR;   // segments per row b: P (features) or 1
  int G;     // segments per tile
  long long nseg, ntiles;
  int tab_lds;  // quantiser tables in LDS
  // LDS carve, byte offsets (multiples of 16)
  unsigned off_tw, off_scale, off_tab, off_idx, bytes;
};

// x h with every product and the sum rounded on its own: what numpy's matmul gives for a row of kron(x, I_N)
QCE_DEV double2 pilot_mul(double2 x, double2 h) {
#pragma clang fp contract(off)
  return make_double2(x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x);
}

// NOISE: 0 none, 1 supplied, 2 generated.  FEAT: 0 y output, 1 features (a.out 1 raw, 2 DFT).
template <int NOISE, int FEAT>
__global__ __launch_bounds__(ROWS_THREADS) void k_observe_rows(QceObserveRowsArgs a, RowsPlan pl) {
  extern __shared__ __attribute__((aligned(16))) char r_smem[];
  double2* T = reinterpret_cast<double2*>(r_smem);                     // G rows of N + 1 (features)
  double2* tw = reinterpret_cast<double2*>(r_smem + pl.off_tw);        // N / 2 (DFT features)
  double* sscale = reinterpret_cast<double*>(r_smem + pl.off_scale);   // S
  double* sthr = reinterpret_cast<double*>(r_smem + pl.off_tab);       // S x nthr, then S x (nthr + 1) labels
  double* slab = sthr + (size_t)a.S * a.nthr;
  int* sidx = reinterpret_cast<int*>(r_smem + pl.off_idx);             // G
  const int tid = threadIdx.x;
  const int N = a.N, M = a.M, nthr = a.nthr, nlab = a.nthr + 1, G = pl.G, SL = pl.SL, SPR = pl.SPR;
  const int RS = N + 1;
  const bool dft = FEAT && a.out == 2;

  for (int i = tid; i < a.S; i += ROWS_THREADS) sscale[i] = a.scales[i];
  if (a.kind == 1 && pl.tab_lds) {
    for (int i = tid; i < a.S * nthr; i += ROWS_THREADS) sthr[i] = a.thr[i];
    for (int i = tid; i < a.S * nlab; i += ROWS_THREADS) slab[i] = a.lab[i];
  }
  if (dft)
    for (int t = tid; t < (N >> 1); t += ROWS_THREADS) {
      double s, c;
      sincospi(-2.0 * (double)t / (double)N, &s, &c);
      tw[t] = make_double2(c, s);
    }
  // (the barrier behind the first tile's SNR indices also covers these tables)

  for (long long tile = blockIdx.x; tile < pl.ntiles; tile += gridDim.x) {
    const long long g0 = tile * G;
    for (int s = tid; s < G; s += ROWS_THREADS) {
      const long long g = g0 + s;
      int idx = 0;
      if (g < pl.nseg) {
        const long long b = g / SPR;
        if (a.idx_in) {
          idx = a.idx_in[b];
          idx = idx < 0 ? 0 : (idx >= a.S ? a.S - 1 : idx);  // device-side indices cannot be checked on the host
        } else if (a.S > 1) {
          const double u = row_uniform(a.seed, a.row_offset + (unsigned long long)b);
          if (a.cdf) {
            for (int i = 0; i < a.S; ++i) idx += a.cdf[i] <= u ? 1 : 0;
          } else {
            idx = (int)(u * (double)a.S);
          }
          idx = idx >= a.S ? a.S - 1 : idx;
        }
        if (g - b * SPR == 0) a.idx_out[b] = idx;
      }
      sidx[s] = idx;
    }
    __syncthreads();

    const int ne = FEAT ? FEAT_TILE : G * SL;
#pragma unroll 4
    for (int e = tid; e < ne; e += ROWS_THREADS) {
      int s, j;
      if (FEAT) {
        s = e >> pl.lgSL;
        j = e & (SL - 1);
      } else {
        s = e / SL;
        j = e - s * SL;
      }
      const long long g = g0 + s;
      if (g >= pl.nseg) {
        if (FEAT) T[s * RS + j] = make_double2(0.0, 0.0);  // rows past the batch transform zeros and store nothing
        continue;
      }
      const long long b = g / SPR;
      const int m = (int)(g - b * SPR) * SL + j;
      const double2* hr = a.h + b * N;
      double2 v;
      if (a.A) {
        const double2* ar = a.A + (long long)m * N;
        v = make_double2(0.0, 0.0);
        for (int c = 0; c < N; ++c) v = cfma(ar[c], hr[c], v);
      } else if (a.P > 0) {
        const int p = m / N;
        v = pilot_mul(a.xk[p], hr[m - p * N]);
      } else {
        v = hr[m];
      }
      double2 wv = make_double2(0.0, 0.0);
      if (NOISE == 1) wv = a.w[b * M + m];
      if (NOISE == 2) wv = cn_draw(a.seed, (a.row_offset + (unsigned long long)b) * (unsigned long long)M + (unsigned)m);
      const int idx = sidx[s];
      const double sc = sscale[idx];
      double2 q;
      if (pl.tab_lds) q = observe_one(v, wv, sc, NOISE != 0, a.kind, sthr + idx * nthr, slab + idx * nlab, nthr);
      else q = observe_one(v, wv, sc, NOISE != 0, a.kind, a.thr + (size_t)idx * nthr, a.lab + (size_t)idx * nlab, nthr);
      if (FEAT) T[s * RS + j] = q;
      else a.y[b * M + m] = q;
    }

    if (FEAT) {
      __syncthreads();
      if (dft) r_fft_rows<ROWS_THREADS>(T, G, N, pl.lgSL, tw);
      const double rs = dft ? 1.0 / sqrt((double)N) : 1.0;
      // row g of the output: 2N floats [Re | Im]; four consecutive floats per thread
      const int q4row = N >> 1;  // float4 groups per row
      for (int e = tid; e < G * q4row; e += ROWS_THREADS) {
        const int s = e / q4row, r = (e - s * q4row) << 2;
        const long long g = g0 + s;
        if (g >= pl.nseg) continue;
        const double2* row = T + s * RS + (r & (N - 1));
        float4 o;
        if (r < N) o = make_float4((float)(row[0].x * rs), (float)(row[1].x * rs), (float)(row[2].x * rs), (float)(row[3].x * rs));
        else o = make_float4((float)(row[0].y * rs), (float)(row[1].y * rs), (float)(row[2].y * rs), (float)(row[3].y * rs));
        *reinterpret_cast<float4*>(a.feat + g * (2LL * N) + r) = o;
      }
    }
    __syncthreads();  // the next tile rewrites sidx and T
  }
}

unsigned up16(size_t v) { return (unsigned)((v + 15) & ~(size_t)15); }

RowsPlan rows_plan(const QceObserveRowsArgs& a) {
  RowsPlan p{};
  const bool feat = a.out != 0;
  p.SL = feat ? a.N : a.M;
  p.lgSL = 0;
  while (feat && (1 << p.lgSL) < a.N) ++p.lgSL;
  p.SPR = feat ? a.M / a.N : 1;
  if (feat) p.G = FEAT_TILE / a.N;
  else {
    p.G = Y_TILE / a.M;
    p.G = p.G < 1 ? 1 : (p.G > MAX_SEGS ? MAX_SEGS : p.G);
  }
  p.nseg = a.B * p.SPR;
  p.ntiles = (p.nseg + p.G - 1) / p.G;
  const size_t tab = a.kind == 1 ? sizeof(double) * (size_t)a.S * (2 * (size_t)a.nthr + 1) : 0;
  p.tab_lds = tab <= QCE_ROWS_TABLE_LDS ? 1 : 0;
  p.off_tw = feat ? up16(sizeof(double2) * (size_t)p.G * (a.N + 1)) : 0;
  p.off_scale = p.off_tw + (feat ? up16(sizeof(double2) * (a.N / 2)) : 0);
  p.off_tab = p.off_scale + up16(sizeof(double) * a.S);
  p.off_idx = p.off_tab + (p.tab_lds ? up16(tab) : 0);
  p.bytes = p.off_idx + up16(sizeof(int) * p.G);
  return p;
}

}  // namespace

bool qce_observe_rows_feature_shape(int N) { return N == 16 || N == 32 || N == 64 || N == 128 || N == 256; }

hipError_t qce_launch_observe_rows(const QceObserveRowsArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.out != 0 && (!qce_observe_rows_feature_shape(a.N) || a.M % a.N)) return hipErrorInvalidValue;
  if (a.S < 1 || a.S > QCE_ROWS_MAX_SNRS) return hipErrorInvalidValue;
  const RowsPlan p = rows_plan(a);
  const dim3 grid((unsigned)(p.ntiles < MAX_BLOCKS ? p.ntiles : MAX_BLOCKS)), block(ROWS_THREADS);
#define QCE_ROWS(NZ, FT) hipLaunchKernelGGL((k_observe_rows<NZ, FT>), grid, block, p.bytes, st, a, p)
  if (a.out == 0) {
    if (a.noise == 0) QCE_ROWS(0, 0);
    else if (a.noise == 1) QCE_ROWS(1, 0);
    else QCE_ROWS(2, 0);
  } else {
    if (a.noise == 0) QCE_ROWS(0, 1);
    else if (a.noise == 1) QCE_ROWS(1, 1);
    else QCE_ROWS(2, 1);
  }
#undef QCE_ROWS
  return hipGetLastError();
}
