// C ABI of libqce.so, estimate side: qce_estimate, qce_log_prob, the K-shard partial entry points and
// qce_weighted_estimate.  Every one switches on the model's kernel family (qce_model::backend); the 'all'-mode
// outputs (final h, (m, s, acc) partials, shifted packed rows) share one dispatcher, run_all.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "qce_capi.h"
#include "qce_common.h"

bool want_f64(const qce_model* m) {
  const char* e = getenv("QCE_KERNEL");
  if (e && strcmp(e, "f64") == 0) return true;
  if (e && (strcmp(e, "h2") == 0 || strcmp(e, "f32") == 0)) return false;
  // an int8 model that fell back (quantiser, shape, structure) is an f64 model in every respect
  if (m->precision == QCE_PRECISION_INT8) return m->backend != QCE_BE_INT8;
  return m->precision == QCE_PRECISION_F64;
}

bool want_int8(const qce_model* m) {
  const char* e = getenv("QCE_KERNEL");
  if (e && (strcmp(e, "f64") == 0 || strcmp(e, "h2") == 0 || strcmp(e, "f32") == 0)) return false;
  return m->precision == QCE_PRECISION_INT8;
}

namespace {

// the batch and shape fields every estimate kernel's argument struct starts with
template <typename Args>
void set_shape(Args& a, const qce_model* m, long long B) {
  a.B = B;
  a.M = m->M;
  a.N = m->N;
  a.K = m->K;
  a.MP = m->MP;
  a.NP = m->NP;
  a.has_mean = m->has_mean;
}

QceEstArgs est_args(qce_model* m, const double2* y, long long B) {
  QceEstArgs a;
  set_shape(a, m, B);
  a.y = y;
  a.pack32 = m->pack32.p;
  a.stride32 = m->stride32;
  a.pack64 = m->pack64.p;
  a.stride64 = m->stride64;
  a.cconst = m->cconst.p;
  return a;
}

int ensure_packs(qce_model* m, hipStream_t st) {
  if (m->packs_valid) return QCE_OK;
  QcePrepareArgs p = m->pack_args;
  if (m->pack64_valid) p.pack64 = nullptr;
  HIPCHK(qce_launch_pack_selective(p, st));
  m->packs_valid = 1;
  m->pack64_valid = 1;
  return QCE_OK;
}

// the FP64 log-prob table alone (k_lp_f64), for the two-pass FP64 'all' path
int ensure_pack64(qce_model* m, hipStream_t st) {
  if (m->packs_valid || m->pack64_valid) return QCE_OK;
  QcePrepareArgs p = m->pack_args;
  p.pack32 = nullptr;
  HIPCHK(qce_launch_pack_selective(p, st));
  m->pack64_valid = 1;
  return QCE_OK;
}

// Inside the fast family: the fp16-split kernels, or (QCE_KERNEL=f32, re-read at every launch: A/B runs flip it
// between estimates of one prepared model) the FP32-MFMA kernels where they cover the shape
bool fast_uses_h2(const qce_model* m) {
  const char* e = getenv("QCE_KERNEL");
  return !(e && strcmp(e, "f32") == 0) || !qce_shape_supported(m->MP, m->NP);
}

// Persistent-grid split of tiles x K (tile, component) items over `slots` resident workgroups: R data-parallel
// rounds of whole tiles, then the remaining tiles' items dealt out stream-K, L to each of nwg workgroups
void streamk_split(long long tiles, long long slots, int K, long long* nwg, long long* R, long long* L) {
  if (tiles >= slots) {
    *nwg = slots;
    *R = tiles / slots;
    *L = ((tiles - *R * slots) * K + *nwg - 1) / *nwg;
  } else {
    *R = 0;
    *L = (tiles * K + slots - 1) / slots;
    if (*L < 1) *L = 1;
    *nwg = (tiles * K + *L - 1) / *L;
  }
}

// 'all' mode in FP64 (qce_estimate_f64.hip): whole tiles data-parallel over one resident workgroup
// per CU, the remaining tiles' (tile, component) items dealt out stream-K; final h, or the FP64
// (m, s, acc) partial when h == nullptr (K-shard path)
int run_f64(qce_model* m, const double2* dy, long long B, double2* h, double* om, double* os, double* oa,
            hipStream_t st, double* pk = nullptr, const double* shift = nullptr) {
  const int g3 = m->backend == QCE_BE_F64_3M ? 1 : (m->backend == QCE_BE_F64_3M_128 ? 2 : 0);  // QceF64Args::g3
  const long long TS = g3 == 2 ? 64LL : (g3 ? 16LL * qce_f64g_waves() : qce_f64_tile(m->MP, m->NP));
  const long long tiles = (B + TS - 1) / TS;
  // one 8-wave workgroup per CU (its ring / y tile fills the LDS), or two 4-wave ones (3M kernel built with 4 waves)
  long long slots = (long long)m->sched_cus() * (g3 == 1 ? 8 / qce_f64g_waves() : 1);
  const char* e = getenv("QCE_WORKGROUPS");
  if (e && atoll(e) > 0) slots = atoll(e);
  long long nwg, R, L;
  streamk_split(tiles, slots, m->K, &nwg, &R, &L);
  QceF64Args a;
  set_shape(a, m, B);
  a.nwg = (int)nwg;
  a.R = (int)R;
  a.L = L;
  a.y = dy;
  a.pack = m->pack_f64.p;
  a.cconst = m->cconst.p;
  a.h = h;
  a.om = om;
  a.os = os;
  a.oa = oa;
  HIPCHK(m->fp_m.ensure((size_t)nwg * 2 * TS));
  HIPCHK(m->fp_s.ensure((size_t)nwg * 2 * TS));
  HIPCHK(m->fp_a.ensure((size_t)nwg * 2 * TS * 2 * m->N));
  a.pm = m->fp_m.p;
  a.ps = m->fp_s.p;
  a.pa = m->fp_a.p;
  a.pk = pk;
  a.shift = shift;
  if (g3 == 1) {
    if (const long long nscr = qce_f64g_scratch_doubles(m->MP, m->NP, m->K, nwg)) {
      HIPCHK(m->fp_scr.ensure((size_t)nscr));
      a.pscr = m->fp_scr.p;
    }
  }
  {
    const char* wv = getenv("QCE_F64_WAVES");  // 8 (default): two waves per SIMD where M, N <= 64
    a.waves = (wv && atoi(wv) == 4) ? 4 : 8;
  }
  a.g3 = g3;
  if (a.g3) a.waves = qce_f64g_waves();
#ifdef QCE_STAMPS
  static unsigned long long* g_stamps = nullptr;
  if (!g_stamps) HIPCHK(hipMalloc(&g_stamps, sizeof(unsigned long long) * 4096 * 8 * 8));
  HIPCHK(hipMemsetAsync(g_stamps, 0, sizeof(unsigned long long) * 4096 * 8 * 8, st));
  a.stamps = nwg <= 4096 ? g_stamps : nullptr;
  g_f64_stamps = g_stamps;
  g_f64_stamp_records = nwg * a.waves;
#endif
  HIPCHK(qce_launch_est_f64(a, h == nullptr, st));
  return QCE_OK;
}

// 'all' mode / K-shard partials in FP64 beyond padded 128 (qce_wsum_f64.hip): lp on FP64 MFMA, the weights of
// the requested output (wmode 0: proba -> h; 1: (m, s, acc); 2: shifted packed rows), the weighted filter sum
int run_wide(qce_model* m, const double2* dy, long long B, int wmode, double2* h, double* om, double* os, double* oa,
             double* pk, const double* shift, hipStream_t st) {
  const size_t BK = (size_t)B * m->K;
  HIPCHK(m->lp_scr.ensure(BK));
  HIPCHK(m->w64_scr.ensure(BK));
  if (int rc = ensure_pack64(m, st)) return rc;
  QceEstArgs a = est_args(m, dy, B);
  HIPCHK(qce_launch_lp(a, m->lp_scr.p, st));
  HIPCHK(qce_launch_wsum_weights(B, m->K, m->lp_scr.p, wmode, shift, m->w64_scr.p, om, os, pk, 2LL * m->N + 2, st));
  QceWsumArgs w;
  set_shape(w, m, B);
  w.y = dy;
  w.pack = m->pack_ws.p;
  w.wT = m->w64_scr.p;
  if (wmode == 0) {
    w.out = h;
    w.ostride = m->N;
    w.ooff = 0;
  } else if (wmode == 1) {
    w.out = reinterpret_cast<double2*>(oa);
    w.ostride = m->N;
    w.ooff = 0;
  } else {
    w.out = reinterpret_cast<double2*>(pk);
    w.ostride = m->N + 1;
    w.ooff = 1;
  }
  HIPCHK(qce_launch_wsum(w, st));
  return QCE_OK;
}

int run_h2x(qce_model* m, const double2* dy, long long B, double2* h, double* om, double* os, float* oa,
            hipStream_t st);

// 'all' mode on the FP16 split kernel, stream-K scheduled over the resident workgroups: final h,
// or the (m, s, acc) partial when h == nullptr (K-shard path)

int run_h2(qce_model* m, const double2* dy, long long B, double2* h, double* om, double* os, float* oa,
           hipStream_t st) {
  if (qce_h2x_shape(m->MP, m->NP)) return run_h2x(m, dy, B, h, om, os, oa, st);
  const long long tiles = (B + 255) / 256;
  long long slots = (long long)m->sched_cus() * qce_h2_blocks_per_cu(m->MP, m->NP, m->has_mean);
  const char* e = getenv("QCE_WORKGROUPS");
  if (e && atoll(e) > 0) slots = atoll(e);
  long long nwg, R, L;
  streamk_split(tiles, slots, m->K, &nwg, &R, &L);
  QceH2Args a;
  set_shape(a, m, B);
  a.nwg = (int)nwg;
  a.R = (int)R;
  a.L = L;
  a.y_scale = m->y_scale;
  a.y = dy;
  a.pack = m->pack16.p;
  a.cstride = m->cstride16;
  a.sinv = m->sinv.p;
  a.cconst = m->cconst.p;
  a.h = h;
  a.om = om;
  a.os = os;
  a.oa = oa;
  HIPCHK(m->sp_m.ensure((size_t)nwg * 2 * 256));
  HIPCHK(m->sp_s.ensure((size_t)nwg * 2 * 256));
  HIPCHK(m->sp_a.ensure((size_t)nwg * 2 * 256 * 2 * m->N));
  HIPCHK(m->yflag.ensure(2));  // inexact flag, largest exponent (k_y_exact)
  a.yflag = m->yflag.p;
  a.pm = m->sp_m.p;
  a.ps = m->sp_s.p;
  a.pa = m->sp_a.p;
  HIPCHK(qce_launch_est_h2(a, h == nullptr, st));
  return QCE_OK;
}

// 'all' mode for the large padded shapes (qce_estimate_h2x.hip): 128-sample tiles x K splits x
// row chunks, split records merged by k_merge_splits
int run_h2x(qce_model* m, const double2* dy, long long B, double2* h, double* om, double* os, float* oa,
            hipStream_t st) {
  const long long tiles = (B + qce_h2x_tile() - 1) / qce_h2x_tile();
  const long long nrc = qce_h2x_row_chunks(m->MP, m->NP);
  const long long slots = m->sched_cus();  // one 128 KB-LDS workgroup per CU
  int ksplit = 1;
  double best = 0.0;
  for (int s = 1; s <= 8 && s <= m->K; ++s) {  // fill the chip: tiles*s*nrc over whole waves of workgroups
    const long long wg = tiles * s * nrc;
    const double eff = (double)wg / (double)(slots * ((wg + slots - 1) / slots));
    if (eff > best + 0.02) {
      best = eff;
      ksplit = s;
    }
  }
  const char* e = getenv("QCE_KSPLIT");
  if (e && atoi(e) > 0) ksplit = atoi(e) < m->K ? atoi(e) : m->K;
  QceH2XArgs a;
  set_shape(a, m, B);
  a.y_scale = m->y_scale;
  HIPCHK(m->yflag.ensure(2));  // inexact flag, largest exponent (k_y_exact)
  a.yflag = m->yflag.p;
  a.y = dy;
  a.pack = m->pack16.p;
  a.cstride = m->cstride16;
  a.sinv = m->sinv.p;
  a.cconst = m->cconst.p;
  a.h = h;
  a.om = om;
  a.os = os;
  a.oa = oa;
  a.rm = a.rs = nullptr;
  a.ra = nullptr;
  if (ksplit > 1) {
    HIPCHK(m->sp_m.ensure((size_t)ksplit * B));
    HIPCHK(m->sp_s.ensure((size_t)ksplit * B));
    HIPCHK(m->sp_a.ensure((size_t)ksplit * B * 2 * m->N));
    a.rm = m->sp_m.p;
    a.rs = m->sp_s.p;
    a.ra = m->sp_a.p;
  }
  HIPCHK(qce_launch_est_h2x(a, ksplit, h == nullptr, st));
  return QCE_OK;
}

QceI8Args i8_args(qce_model* m, const double2* dy, long long B) {
  QceI8Args a;
  set_shape(a, m, B);
  a.S = m->i8_S;
  a.group = m->i8_group;
  a.y_scale = m->y_scale;
  a.y = dy;
  a.planes = m->i8_planes.p;
  a.pstride = qce_pack_i8_bytes(m->MP, m->NP, m->i8_S);
  a.rowtab = m->i8_rowtab.p;
  a.cconst = m->cconst.p;
  a.h = nullptr;
  return a;
}

// 'all' mode on the int8 digit planes (qce_estimate_i8.hip): one workgroup per sample tile, final h only
int run_i8(qce_model* m, const double2* dy, long long B, double2* h, hipStream_t st) {
  QceI8Args a = i8_args(m, dy, B);
  a.h = h;
  HIPCHK(qce_launch_est_i8(a, st));
  return QCE_OK;
}

}  // namespace

int run_i8_debug(qce_model* m, const double2* dy, long long B, int k, double* rawL, double* rawW, hipStream_t st) {
  QceI8Args a = i8_args(m, dy, B);
  a.dbg_k = k;
  a.dbgL = rawL;
  a.dbgW = rawW;
  HIPCHK(qce_launch_est_i8(a, st));
  return QCE_OK;
}

// stage host input (io == HOST) or use the device pointer directly
int stage_input(qce_model* m, const double* y, long long B, int io, hipStream_t st, const double2** dy) {
  if (io == QCE_IO_DEVICE) {
    *dy = reinterpret_cast<const double2*>(y);
    return QCE_OK;
  }
  HIPCHK(m->y_scr.ensure((size_t)B * m->M));
  HIPCHK(hipMemcpyAsync(m->y_scr.p, y, sizeof(double2) * (size_t)B * m->M, hipMemcpyHostToDevice, st));
  *dy = m->y_scr.p;
  return QCE_OK;
}

QceFftpEstArgs fftp_args(qce_model* m, const double2* y, long long B) {
  QceFftpEstArgs a;
  a.B = B;
  a.N = m->N;
  a.n1 = m->fft_n1;
  a.n2 = m->fft_n2;
  a.K = m->K;
  a.Kp = qce_fftp_kpad(m->K);
  a.P = m->fp_P;
  a.has_mean = m->has_mean;
  a.y = y;
  a.tabL = m->fp_tabL.p;
  a.cprime = m->fp_cprime.p;
  a.tabW = m->fp_tabW.p;
  a.wts = nullptr;
  a.h = nullptr;
  a.lp = nullptr;
  return a;
}

QceFftEstArgs fft_args(qce_model* m, const double2* y, long long B) {
  QceFftEstArgs a;
  a.B = B;
  a.N = m->N;
  a.n1 = m->fft_n1;
  a.n2 = m->fft_n2;
  a.K = m->K;
  a.has_mean = m->has_mean;
  a.y = y;
  a.rinvT = m->f_rinvT.p;
  a.uT = m->f_uT.p;
  a.cprime = m->f_cprime.p;
  a.wT = m->f_wT.p;
  a.bT = m->f_bT.p;
  a.wts = nullptr;
  a.h = nullptr;
  a.lp = nullptr;
  a.om = a.os = nullptr;
  a.oa = nullptr;
  a.Kp = qce_fft_kpad(m->K);
  a.pr = m->f_pr.p;
  a.pur = m->f_pur.p;
  a.pui = m->f_pui.p;
  a.pc = m->f_pc.p;
  a.pw = m->f_pw.p;
  a.pbr = m->f_pbr.p;
  a.pbi = m->f_pbi.p;
  a.cu = m->sched_cus();
  return a;
}

namespace {

// qce_estimate's mode / mode_param as k_select takes them: kmode 0 'all', 1 top-n, 2 cumulative-p, 3 argmax
int parse_mode(int mode, double mode_param, int* kmode, int* n, double* p) {
  *kmode = 0;
  *n = 0;
  *p = 0.0;
  if (mode == QCE_MODE_TOPN) {
    if (mode_param < 1.0 || mode_param != floor(mode_param))
      return qce_set_error(QCE_EARG, "top-n needs an integer n >= 1");
    *n = mode_param > 1e9 ? 1000000000 : (int)mode_param;
    *kmode = (*n == 1) ? 3 : 1;
  } else if (mode == QCE_MODE_CUMP) {
    *kmode = 2;
    *p = mode_param;
  } else if (mode != QCE_MODE_ALL) {
    return qce_set_error(QCE_EARG, "unknown mode");
  }
  return QCE_OK;
}

// What one 'all'-mode pass over a batch writes (device pointers; the fields of the other kinds stay null)
struct AllOut {
  enum Kind { FINAL, PARTIAL_F32, PARTIAL_F64, SHIFTED } kind;
  double2* h = nullptr;                 // FINAL: the estimate (B x N)
  double *om = nullptr, *os = nullptr;  // PARTIAL_*: per-row running max and sum of the shard's components
  void* oa = nullptr;                   // PARTIAL_*: the accumulator (B x 2N), float or double as the kind says
  double* pk = nullptr;                 // SHIFTED: packed rows [s e^{m - shift}, 0, acc e^{m - shift}] (B x (2N + 2))
  const double* shift = nullptr;
};

// The 'all'-mode pass of every family, for every output.  Accumulators: the Fourier kernels write either width, the
// FP64 families (big, fused, wide) a double one and shifted rows, the fast family a float one; what a family does not
// write itself is converted here, each conversion once.
int run_all(qce_model* m, const double2* dy, long long B, const AllOut& o, hipStream_t st) {
  const QceBackend be = m->backend;
  const bool f64_family = be == QCE_BE_BIG || be == QCE_BE_F64_4M || be == QCE_BE_F64_3M ||
                          be == QCE_BE_F64_3M_128 || be == QCE_BE_F64_WIDE;
  const long long nacc = B * 2 * m->N;
  if (be == QCE_BE_INT8 && o.kind != AllOut::FINAL)
    return qce_set_error(QCE_ENOTIMPL, "K-shard partials are not covered by the int8 precision");
  if (be == QCE_BE_FOURIER_PILOTS && o.kind != AllOut::FINAL)
    return qce_set_error(QCE_ENOTIMPL, "K-shard partials are not covered by the Fourier path with pilots "
                                       "(QCE_OPT_FOURIER_PILOTS)");
  if (o.kind == AllOut::SHIFTED && !f64_family) {  // their (m, s, acc) partial, scaled and packed
    HIPCHK(m->m_scr.ensure((size_t)B));
    HIPCHK(m->s_scr.ensure((size_t)B));
    HIPCHK(m->part_a64.ensure((size_t)nacc));
    AllOut part{AllOut::PARTIAL_F64};
    part.om = m->m_scr.p;
    part.os = m->s_scr.p;
    part.oa = m->part_a64.p;
    if (int rc = run_all(m, dy, B, part, st)) return rc;
    HIPCHK(qce_launch_pack_shifted(B, m->N, m->m_scr.p, m->s_scr.p, m->part_a64.p, nullptr, o.shift, o.pk, st));
    return QCE_OK;
  }
  if (o.kind == AllOut::PARTIAL_F32 && f64_family) {  // FP64 partial, rounded to the f32 accumulator
    HIPCHK(m->part_a64.ensure((size_t)nacc));
    AllOut wide = o;
    wide.kind = AllOut::PARTIAL_F64;
    wide.oa = m->part_a64.p;
    if (int rc = run_all(m, dy, B, wide, st)) return rc;
    HIPCHK(qce_launch_f64_to_f32(m->part_a64.p, static_cast<float*>(o.oa), nacc, st));
    return QCE_OK;
  }
  if (o.kind == AllOut::PARTIAL_F64 && be == QCE_BE_FAST) {  // the fast path keeps an f32 accumulator: widen it
    HIPCHK(m->acc_scr.ensure((size_t)nacc));
    AllOut narrow = o;
    narrow.kind = AllOut::PARTIAL_F32;
    narrow.oa = m->acc_scr.p;
    if (int rc = run_all(m, dy, B, narrow, st)) return rc;
    HIPCHK(qce_launch_f32_to_f64(m->acc_scr.p, static_cast<double*>(o.oa), nacc, st));
    return QCE_OK;
  }
  const int wmode = o.kind == AllOut::FINAL ? 0 : (o.kind == AllOut::SHIFTED ? 2 : 1);  // run_wide / qce_big_partial
  switch (be) {
    case QCE_BE_NONE: break;
    case QCE_BE_FOURIER: {  // qce_fft.hip / qce_fft_mfma.hip: modes 0 (h), 3 (f32 partial), 4 (f64 partial)
      QceFftEstArgs fa = fft_args(m, dy, B);
      fa.h = o.h;
      fa.om = o.om;
      fa.os = o.os;
      fa.oa = static_cast<float*>(o.oa);  // mode 4 writes doubles through it
      const int fmode = o.kind == AllOut::FINAL ? 0 : (o.kind == AllOut::PARTIAL_F32 ? 3 : 4);
      if (m->fft_mfma) HIPCHK(qce_launch_fft_mfma(fa, fmode, st));
      else HIPCHK(qce_launch_fft_est(fa, fmode, st));
      return QCE_OK;
    }
    case QCE_BE_BIG:  // N or M beyond 256: lp GEMM -> FP64 weights -> stacked-filter GEMM (qce_big.hip)
      if (o.kind != AllOut::FINAL)
        return qce_big_partial(m, dy, B, wmode, o.om, o.os, static_cast<double*>(o.oa), o.pk, o.shift, st);
      HIPCHK(m->lp_scr.ensure((size_t)B * m->K));
      HIPCHK(m->w64_scr.ensure((size_t)B * m->K));
      if (int rc = qce_big_lp(m, dy, B, m->lp_scr.p, st)) return rc;
      if (m->K > qce_select_max_k()) {  // 'all' takes any K
        if (int rc = qce_big_proba(m, B, st)) return rc;
      } else {  // responsibilities = proba (:220-228: no renormalisation)
        HIPCHK(qce_launch_select(B, m->K, m->lp_scr.p, 0, 0, 0.0, m->w64_scr.p, nullptr, nullptr, st));
      }
      return qce_big_wsum(m, dy, B, m->w64_scr.p, o.h, m->N, st);
    case QCE_BE_F64_4M:
    case QCE_BE_F64_3M:
    case QCE_BE_F64_3M_128:
      return run_f64(m, dy, B, o.h, o.om, o.os, static_cast<double*>(o.oa), st, o.pk, o.shift);
    case QCE_BE_F64_WIDE:
      return run_wide(m, dy, B, wmode, o.h, o.om, o.os, static_cast<double*>(o.oa), o.pk, o.shift, st);
    case QCE_BE_INT8:
      return run_i8(m, dy, B, o.h, st);
    case QCE_BE_FOURIER_PILOTS: {  // qce_fft_pilot.hip: final h only
      QceFftpEstArgs fa = fftp_args(m, dy, B);
      fa.h = o.h;
      HIPCHK(qce_launch_fftp_est(fa, 0, st));
      return QCE_OK;
    }
    case QCE_BE_FAST: {
      if (fast_uses_h2(m)) return run_h2(m, dy, B, o.h, o.om, o.os, static_cast<float*>(o.oa), st);
      if (int rc = ensure_packs(m, st)) return rc;
      QceEstArgs a = est_args(m, dy, B);
      if (o.kind == AllOut::FINAL) HIPCHK(qce_launch_est_all(a, o.h, st));
      else HIPCHK(qce_launch_est_partial(a, o.om, o.os, static_cast<float*>(o.oa), st));
      return QCE_OK;
    }
  }
  return qce_set_error(QCE_ESTATE, "qce_prepare has not been called on this model");
}

// h_b = sum_k w[b][k] (W_k y_b + b_k) with FP64 weights on the device: the Fourier kernel's weighted output, the
// stacked-filter GEMM, or the FP64 sparse kernel over the dense filters
int weighted_sum(qce_model* m, const double2* y, long long B, const double* w, double2* h, hipStream_t st) {
  if (m->backend == QCE_BE_FOURIER) {
    QceFftEstArgs fa = fft_args(m, y, B);
    fa.wts = w;
    fa.h = h;
    HIPCHK(qce_launch_fft_est(fa, 2, st));
    return QCE_OK;
  }
  if (m->backend == QCE_BE_FOURIER_PILOTS) {
    QceFftpEstArgs fa = fftp_args(m, y, B);
    fa.wts = w;
    fa.h = h;
    HIPCHK(qce_launch_fftp_est(fa, 2, st));
    return QCE_OK;
  }
  if (m->backend == QCE_BE_BIG) return qce_big_wsum(m, y, B, w, h, m->N, st);
  HIPCHK(m->WT.ensure((size_t)m->K * m->M * m->N));
  HIPCHK(qce_launch_sparse_f64(B, m->N, m->M, m->K, y, w, m->W.p, m->bvec.p, m->WT.p, !m->wt_valid, h, st));
  m->wt_valid = 1;
  return QCE_OK;
}

// qce_estimate_partial (f32 accumulator) and qce_estimate_partial_f64
int partial_impl(qce_model* m, const double* y, int64_t B, double* m_out, double* s_out, void* acc_out, bool f64,
                 int io, void* stream) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (B < 0 || (B > 0 && (!y || !m_out || !s_out || !acc_out))) return qce_set_error(QCE_EARG, "bad arguments");
  if (B == 0) return QCE_OK;
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  const double2* dy = nullptr;
  if ((rc = stage_input(m, y, B, io, st, &dy))) return rc;
  const size_t nacc = (size_t)B * 2 * m->N;
  AllOut o{f64 ? AllOut::PARTIAL_F64 : AllOut::PARTIAL_F32};
  o.om = m_out;
  o.os = s_out;
  o.oa = acc_out;
  if (io == QCE_IO_HOST) {
    HIPCHK(m->m_scr.ensure((size_t)B));
    HIPCHK(m->s_scr.ensure((size_t)B));
    HIPCHK(f64 ? m->part_a64.ensure(nacc) : m->acc_scr.ensure(nacc));
    o.om = m->m_scr.p;
    o.os = m->s_scr.p;
    o.oa = f64 ? static_cast<void*>(m->part_a64.p) : static_cast<void*>(m->acc_scr.p);
  }
  if ((rc = run_all(m, dy, B, o, st))) return rc;
  if (io == QCE_IO_HOST) {
    HIPCHK(hipMemcpyAsync(m_out, o.om, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s_out, o.os, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(acc_out, o.oa, (f64 ? sizeof(double) : sizeof(float)) * nacc, hipMemcpyDeviceToHost, st));
    HOST_SYNC_CHECK(m, st);
  }
  return QCE_OK;
}

}  // namespace

int backend_lp(qce_model* m, const double2* x, long long B, double* lp, hipStream_t st) {
  if (m->backend == QCE_BE_FOURIER) {
    QceFftEstArgs fa = fft_args(m, x, B);
    fa.lp = lp;
    HIPCHK(qce_launch_fft_est(fa, 1, st));
    return QCE_OK;
  }
  if (m->backend == QCE_BE_FOURIER_PILOTS) {
    QceFftpEstArgs fa = fftp_args(m, x, B);
    fa.lp = lp;
    HIPCHK(qce_launch_fftp_est(fa, 1, st));
    return QCE_OK;
  }
  if (m->backend == QCE_BE_BIG) return qce_big_lp(m, x, B, lp, st);
  if (int rc = ensure_packs(m, st)) return rc;
  QceEstArgs a = est_args(m, x, B);
  HIPCHK(qce_launch_lp(a, lp, st));
  return QCE_OK;
}

extern "C" {

int qce_estimate(qce_model* m, const double* y, int64_t B, int mode, double mode_param, double* h_out, int io,
                 void* stream) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (B < 0 || (B > 0 && (!y || !h_out))) return qce_set_error(QCE_EARG, "bad y / h_out");
  if (B == 0) return QCE_OK;
  const QceBackend be = m->backend;
  const bool dense = !qce_be_fourier(be) && be != QCE_BE_BIG;  // the fused-kernel families over padded tables
  if (dense && mode != QCE_MODE_ALL && !qce_select_shape_supported(m->MP, m->NP))
    return qce_set_error(QCE_ENOTIMPL, "selective modes: shape not covered");
  if (mode != QCE_MODE_ALL && m->K > qce_select_max_k())
    return qce_set_error(QCE_ENOTIMPL, "selective modes support K <= " + std::to_string(qce_select_max_k()));
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  if (io == QCE_IO_HOST)
    if (const long long C = host_chunk_rows(m, B))
      return estimate_host_chunked(m, y, B, C, mode, mode_param, h_out, st);
  const double2* dy = nullptr;
  if ((rc = stage_input(m, y, B, io, st, &dy))) return rc;
  double2* dh = reinterpret_cast<double2*>(h_out);
  if (io == QCE_IO_HOST) {
    HIPCHK(m->h_scr.ensure((size_t)B * m->N));
    dh = m->h_scr.p;
  }
  int kmode, n;
  double p;
  if ((rc = parse_mode(mode, mode_param, &kmode, &n, &p))) return rc;
  if (mode == QCE_MODE_ALL) {
    AllOut o{AllOut::FINAL};
    o.h = dh;
    if ((rc = run_all(m, dy, B, o, st))) return rc;
  } else {
    const size_t BK = (size_t)B * m->K;
    HIPCHK(m->lp_scr.ensure(BK));
    if ((rc = backend_lp(m, dy, B, m->lp_scr.p, st))) return rc;
    if (dense && !want_f64(m)) {  // f32 selection weights into the FP32-MFMA weighted kernel
      HIPCHK(m->w_scr.ensure(BK));
      HIPCHK(qce_launch_select(B, m->K, m->lp_scr.p, kmode, n, p, nullptr, nullptr, m->w_scr.p, st));
      HIPCHK(qce_launch_est_weighted(est_args(m, dy, B), m->w_scr.p, dh, st));
    } else {
      // FP64 selection weights and FP64 filters: the reference sorts complex128-derived proba
      // (gmm_cplx_bussgang.py:213, :235-236)
      HIPCHK(m->w64_scr.ensure(BK));
      HIPCHK(qce_launch_select(B, m->K, m->lp_scr.p, kmode, n, p, nullptr, nullptr, nullptr, st, m->w64_scr.p));
      if ((rc = weighted_sum(m, dy, B, m->w64_scr.p, dh, st))) return rc;
    }
  }
  if (io == QCE_IO_HOST) {
    HIPCHK(hipMemcpyAsync(h_out, dh, sizeof(double2) * (size_t)B * m->N, hipMemcpyDeviceToHost, st));
    HOST_SYNC_CHECK(m, st);
  }
  return QCE_OK;
}

int qce_log_prob(qce_model* m, const double* X, int64_t B, double* lp_out, double* proba_out, int64_t* labels_out,
                 int io, void* stream) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (B < 0 || (B > 0 && !X)) return qce_set_error(QCE_EARG, "bad X");
  if (B == 0) return QCE_OK;
  if (m->K > qce_select_max_k() && (proba_out || labels_out))
    return qce_set_error(QCE_ENOTIMPL, "proba/labels support K <= " + std::to_string(qce_select_max_k()));
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  const double2* dx = nullptr;
  if ((rc = stage_input(m, X, B, io, st, &dx))) return rc;
  const size_t BK = (size_t)B * m->K;
  double* dlp = lp_out;
  double* dpr = proba_out;
  long long* dlab = reinterpret_cast<long long*>(labels_out);
  if (io == QCE_IO_HOST || !lp_out) {
    HIPCHK(m->lp_scr.ensure(BK));
    dlp = m->lp_scr.p;
  }
  if (io == QCE_IO_HOST && proba_out) {
    HIPCHK(m->proba_scr.ensure(BK));
    dpr = m->proba_scr.p;
  }
  if (io == QCE_IO_HOST && labels_out) {
    HIPCHK(m->lab_scr.ensure((size_t)B));
    dlab = m->lab_scr.p;
  }
  if ((rc = backend_lp(m, dx, B, dlp, st))) return rc;
  if (proba_out || labels_out) HIPCHK(qce_launch_select(B, m->K, dlp, 0, 0, 0.0, dpr, dlab, nullptr, st));
  if (io == QCE_IO_HOST) {
    if (lp_out) HIPCHK(hipMemcpyAsync(lp_out, dlp, sizeof(double) * BK, hipMemcpyDeviceToHost, st));
    if (proba_out) HIPCHK(hipMemcpyAsync(proba_out, dpr, sizeof(double) * BK, hipMemcpyDeviceToHost, st));
    if (labels_out) HIPCHK(hipMemcpyAsync(labels_out, dlab, sizeof(int64_t) * B, hipMemcpyDeviceToHost, st));
    HOST_SYNC_CHECK(m, st);
  }
  return QCE_OK;
}

int qce_estimate_partial(qce_model* m, const double* y, int64_t B, double* m_out, double* s_out, float* acc_out,
                         int io, void* stream) {
  return partial_impl(m, y, B, m_out, s_out, acc_out, false, io, stream);
}

int qce_estimate_partial_f64(qce_model* m, const double* y, int64_t B, double* m_out, double* s_out, double* acc_out,
                             int io, void* stream) {
  return partial_impl(m, y, B, m_out, s_out, acc_out, true, io, stream);
}

int qce_estimate_partial_shifted(qce_model* m, const double* y, int64_t B, const double* shift, double* packed_out,
                                 int io, void* stream) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (B < 0 || (B > 0 && (!y || !packed_out || !shift))) return qce_set_error(QCE_EARG, "bad arguments");
  if (B == 0) return QCE_OK;
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  const double2* dy = nullptr;
  if ((rc = stage_input(m, y, B, io, st, &dy))) return rc;
  const size_t W = (size_t)B * (2 * m->N + 2);
  AllOut o{AllOut::SHIFTED};
  o.pk = packed_out;
  o.shift = shift;
  if (io == QCE_IO_HOST) {
    HIPCHK(m->fp_pack.ensure(W));
    o.pk = m->fp_pack.p;
    HIPCHK(m->shift_scr.ensure(1));
    HIPCHK(hipMemcpyAsync(m->shift_scr.p, shift, sizeof(double), hipMemcpyHostToDevice, st));
    o.shift = m->shift_scr.p;
  }
  if ((rc = run_all(m, dy, B, o, st))) return rc;
  if (io == QCE_IO_HOST) {
    HIPCHK(hipMemcpyAsync(packed_out, o.pk, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    HOST_SYNC_CHECK(m, st);
  }
  return QCE_OK;
}

}  // extern "C"

// Selective-mode LMMSE sum with weights computed elsewhere (the K-shard path's globally selected weights of
// this shard's components): h_b = sum_k w[b][k] (W_k y_b + b_k) (gmm_cplx_bussgang.py:216-218, :239-241 for one
// shard of the sum).
int qce_weighted_estimate(qce_model* m, const double2* y, long long B, const double* w, double2* h, hipStream_t st) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (B <= 0) return QCE_OK;
  DeviceGuard g(m->device);
  return weighted_sum(m, y, B, w, h, st);
}
