// C ABI of libqce.so, host-I/O side of qce_estimate: pinned host memory for callers, and the two chunked pipelines
// that overlap a large host batch's transfers with its kernels (each chunk is a device-I/O qce_estimate).
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "qce_capi.h"

namespace {

// memcpy split over a few host threads (pageable numpy buffer <-> pinned slot)
void par_memcpy(void* dst, const void* src, size_t bytes) {
  const size_t piece = (size_t)2 << 20;
  int nt = (int)((bytes + piece - 1) / piece);
  static const int cap = [] {  // QCE_HOST_THREADS (default 16: the CPU share of one GPU on an 8-GPU node)
    const char* v = getenv("QCE_HOST_THREADS");
    const int hw = (int)std::thread::hardware_concurrency();
    int c = v ? atoi(v) : 16;
    if (hw > 0 && c > hw) c = hw;
    return c < 1 ? 1 : c;
  }();
  if (nt > cap) nt = cap;
  if (nt <= 1) {
    memcpy(dst, src, bytes);
    return;
  }
  const size_t per = (bytes + nt - 1) / nt;
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) {
    const size_t o = per * t;
    if (o >= bytes) break;
    const size_t n = (o + per > bytes) ? bytes - o : per;
    th.emplace_back([=] { memcpy((char*)dst + o, (const char*)src + o, n); });
  }
  memcpy(dst, src, per < bytes ? per : bytes);
  for (auto& x : th) x.join();
}

}  // namespace

// rows per host-pipeline chunk; 0 = one shot (QCE_HOST_PIPELINE=0, or too small a batch to split)
long long host_chunk_rows(const qce_model* m, long long B) {
  const char* e = getenv("QCE_HOST_PIPELINE");
  if (e && e[0] == '0') return 0;
  const long long width = m->M > m->N ? m->M : m->N;
  long long cap = ((long long)32 << 20) / (16 * width);  // <= 32 MB per slot and direction
  static const long long parts = [] {  // QCE_HOST_CHUNKS: chunks per batch (A/B runs; default 8)
    const char* v = getenv("QCE_HOST_CHUNKS");
    const long long n = v ? atoll(v) : 8;
    return n < 2 ? 2 : n;
  }();
  long long c = (B + parts - 1) / parts;
  if (c > cap) c = cap;
  c = (c + 255) / 256 * 256;
  if (c < 4096) c = 4096;
  return (B >= 2 * c) ? c : 0;
}

namespace {

// Host memory the GPU can DMA directly: already page-locked (hipHostMalloc'ed, or registered by the caller), or
// registered here for the duration of one call (hipHostRegister pins the pages the caller's array already has:
// ~0.3 ms per 100 MB of touched memory, measured on the box, profiles/r05_hostreg_probe.json).
struct HostDma {
  void* p = nullptr;
  bool registered = false;  // registered by this call: unregistered at its end
  bool ok = false;
  HostDma(void* ptr, size_t bytes) : p(ptr) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess && at.type == hipMemoryTypeHost) {
      ok = true;
      return;
    }
    (void)hipGetLastError();
    if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess) {
      ok = registered = true;
      return;
    }
    (void)hipGetLastError();  // e.g. a range overlapping another registration: the staged path takes it
  }
  ~HostDma() {
    if (registered) (void)hipHostUnregister(p);
  }
};

// row boundaries of the direct-DMA pipeline: chunks growing x4 from the first (whose upload is the only exposed
// transfer) to the middle and shrinking again (the last chunk's download is the other); an upload of 1 KB rows at
// ~56 GB/s is ~5x faster than the estimate of a row, so each upload hides behind the previous chunk's kernel
std::vector<long long> direct_chunks(long long B) {
  std::vector<long long> sz;
  const char* e0 = getenv("QCE_HOST_C0");  // first chunk's rows (A/B runs; default B / 24)
  const char* eg = getenv("QCE_HOST_GROW");  // growth factor of the chunks towards the middle (default 4)
  long long c0 = e0 ? atoll(e0) : B / 24;
  const long long grow = eg && atoll(eg) >= 1 ? atoll(eg) : 4;
  if (c0 < 4096) c0 = 4096;
  long long left = B;
  std::vector<long long> head, tail;
  for (long long c = c0; left > 0;) {
    if (left <= 2 * c) {
      head.push_back(left);
      left = 0;
      break;
    }
    head.push_back(c);
    tail.push_back(c);
    left -= 2 * c;
    c *= grow;
  }
  sz = head;
  for (auto it = tail.rbegin(); it != tail.rend(); ++it) sz.push_back(*it);
  std::vector<long long> bounds{0};
  for (long long v : sz) bounds.push_back(bounds.back() + v);
  return bounds;
}

// Every return of a host-I/O pipeline, the error paths included, first waits for its copy streams: the
// caller's arrays are unregistered (HostDma) or handed back right after, and an async copy may still be using them.
struct CopyStreamsDrain {
  hipStream_t a, b;
  ~CopyStreamsDrain() {
    if (a) (void)hipStreamSynchronize(a);
    if (b) (void)hipStreamSynchronize(b);
  }
};
// the copy-in / copy-out streams and the events of both pipelines, created on first use
int pipeline_streams(qce_model* m) {
  auto& hp = m->hp;
  if (!hp.s_in) HIPCHK(hipStreamCreateWithFlags(&hp.s_in, hipStreamNonBlocking));
  if (!hp.s_out) HIPCHK(hipStreamCreateWithFlags(&hp.s_out, hipStreamNonBlocking));
  for (hipEvent_t* ev : {hp.ev_in, hp.ev_c, hp.ev_out})
    for (int i = 0; i < 2; ++i)
      if (!ev[i]) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  return QCE_OK;
}

// estimate_host_direct could not get its whole-batch device scratch: the bounded staged pipeline takes the batch
constexpr int kDirectNoScratch = -1;

// Host numpy I/O straight from / into the caller's arrays (both DMA-able, see HostDma): per chunk H2D on a copy
// stream, the estimate on the compute stream, D2H on a second copy stream -- no host copies, one sync at the end.
int estimate_host_direct(qce_model* m, const double* y, long long B, int mode, double mode_param, double* h_out,
                         hipStream_t st) {
  auto& hp = m->hp;
  const size_t M = (size_t)m->M, N = (size_t)m->N;
  if (int rc = pipeline_streams(m)) return rc;
  if (m->y_scr.ensure((size_t)B * M) != hipSuccess || m->h_scr.ensure((size_t)B * N) != hipSuccess) {
    (void)hipGetLastError();
    m->y_scr.release();  // the staged pipeline sizes its own (bounded) scratch
    m->h_scr.release();
    return kDirectNoScratch;
  }
  CopyStreamsDrain drain{hp.s_in, hp.s_out};
  const std::vector<long long> bd = direct_chunks(B);
  const double2* ys = reinterpret_cast<const double2*>(y);
  double2* hs = reinterpret_cast<double2*>(h_out);
  // the copy streams start behind the compute stream's earlier work (the scratch buffers' previous readers)
  HIPCHK(hipEventRecord(hp.ev_c[1], st));
  HIPCHK(hipStreamWaitEvent(hp.s_in, hp.ev_c[1], 0));
  int rc = QCE_OK;
  for (size_t i = 0; i + 1 < bd.size() && rc == QCE_OK; ++i) {
    const long long o = bd[i], n = bd[i + 1] - bd[i];
    HIPCHK(hipMemcpyAsync(m->y_scr.p + o * M, ys + o * M, sizeof(double2) * (size_t)n * M, hipMemcpyHostToDevice,
                          hp.s_in));
    HIPCHK(hipEventRecord(hp.ev_in[0], hp.s_in));
    HIPCHK(hipStreamWaitEvent(st, hp.ev_in[0], 0));
    rc = qce_estimate(m, reinterpret_cast<const double*>(m->y_scr.p + o * M), n, mode, mode_param,
                      reinterpret_cast<double*>(m->h_scr.p + o * N), QCE_IO_DEVICE, st);
    if (rc != QCE_OK) break;
    HIPCHK(hipEventRecord(hp.ev_c[0], st));
    HIPCHK(hipStreamWaitEvent(hp.s_out, hp.ev_c[0], 0));
    HIPCHK(hipMemcpyAsync(hs + o * N, m->h_scr.p + o * N, sizeof(double2) * (size_t)n * N, hipMemcpyDeviceToHost,
                          hp.s_out));
  }
  HIPCHK(hipStreamSynchronize(hp.s_in));
  HIPCHK(hipStreamSynchronize(hp.s_out));
  if (rc) return rc;
  HOST_SYNC_CHECK(m, st);
  return QCE_OK;
}

// Host numpy I/O split into chunks: host copies into a pinned slot, H2D on a copy stream, the estimate on
// the compute stream, D2H on a second copy stream into another pinned slot, host copy out -- chunk i's
// transfers overlap chunk i-1's and i+1's compute (results identical: every sample is independent).
int estimate_host_pipelined(qce_model* m, const double* y, long long B, long long C, int mode, double mode_param,
                            double* h_out, hipStream_t st) {
  auto& hp = m->hp;
  const size_t M = (size_t)m->M, N = (size_t)m->N;
  if (int rc = pipeline_streams(m)) return rc;
  CopyStreamsDrain drain{hp.s_in, hp.s_out};
  if (hp.cap_y < (size_t)C * M || hp.cap_h < (size_t)C * N) {
    HIPCHK(hipStreamSynchronize(hp.s_in));
    HIPCHK(hipStreamSynchronize(hp.s_out));
    for (int i = 0; i < 2; ++i) {
      if (hp.pin_y[i]) (void)hipHostFree(hp.pin_y[i]);
      if (hp.pin_h[i]) (void)hipHostFree(hp.pin_h[i]);
      hp.pin_y[i] = hp.pin_h[i] = nullptr;
    }
    hp.cap_y = hp.cap_h = 0;
    for (int i = 0; i < 2; ++i) {
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hp.pin_y[i]), sizeof(double2) * (size_t)C * M, hipHostMallocDefault));
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hp.pin_h[i]), sizeof(double2) * (size_t)C * N, hipHostMallocDefault));
    }
    hp.cap_y = (size_t)C * M;
    hp.cap_h = (size_t)C * N;
  }
  // two device slots per direction, like the pinned ones (bounded scratch: a batch of any size streams through)
  HIPCHK(m->y_scr.ensure((size_t)2 * C * M));
  HIPCHK(m->h_scr.ensure((size_t)2 * C * N));
  const long long nc = (B + C - 1) / C;
  const double2* ys = reinterpret_cast<const double2*>(y);
  double2* hs = reinterpret_cast<double2*>(h_out);
  // the copy-in stream starts behind the compute stream's earlier work (the scratch slots' previous readers)
  HIPCHK(hipEventRecord(hp.ev_c[0], st));
  HIPCHK(hipStreamWaitEvent(hp.s_in, hp.ev_c[0], 0));
  int rc = QCE_OK;
  for (long long i = 0; i <= nc; ++i) {
    if (i < nc && rc == QCE_OK) {
      const int s = (int)(i & 1);
      const long long o = i * C, n = (B - o) < C ? (B - o) : C;
      double2* yslot = m->y_scr.p + (size_t)s * C * M;
      double2* hslot = m->h_scr.p + (size_t)s * C * N;
      if (i >= 2) HIPCHK(hipEventSynchronize(hp.ev_in[s]));  // slot s: chunk i-2's upload has read it
      par_memcpy(hp.pin_y[s], ys + o * M, sizeof(double2) * (size_t)n * M);
      if (i >= 2) HIPCHK(hipStreamWaitEvent(hp.s_in, hp.ev_c[s], 0));  // chunk i-2's estimate has read y slot s
      HIPCHK(hipMemcpyAsync(yslot, hp.pin_y[s], sizeof(double2) * (size_t)n * M, hipMemcpyHostToDevice, hp.s_in));
      HIPCHK(hipEventRecord(hp.ev_in[s], hp.s_in));
      HIPCHK(hipStreamWaitEvent(st, hp.ev_in[s], 0));
      if (i >= 2) HIPCHK(hipStreamWaitEvent(st, hp.ev_out[s], 0));  // chunk i-2's download has read h slot s
      rc = qce_estimate(m, reinterpret_cast<const double*>(yslot), n, mode, mode_param,
                        reinterpret_cast<double*>(hslot), QCE_IO_DEVICE, st);
      if (rc == QCE_OK) {
        HIPCHK(hipEventRecord(hp.ev_c[s], st));
        HIPCHK(hipStreamWaitEvent(hp.s_out, hp.ev_c[s], 0));
        HIPCHK(hipMemcpyAsync(hp.pin_h[s], hslot, sizeof(double2) * (size_t)n * N, hipMemcpyDeviceToHost,
                              hp.s_out));
        HIPCHK(hipEventRecord(hp.ev_out[s], hp.s_out));
      }
    }
    if (i >= 1 && rc == QCE_OK) {  // chunk i-1 back to the caller's array
      const long long j = i - 1, o = j * C, n = (B - o) < C ? (B - o) : C;
      const int s = (int)(j & 1);
      HIPCHK(hipEventSynchronize(hp.ev_out[s]));
      par_memcpy(hs + o * N, hp.pin_h[s], sizeof(double2) * (size_t)n * N);
    }
  }
  HIPCHK(hipStreamSynchronize(hp.s_in));
  HIPCHK(hipStreamSynchronize(hp.s_out));
  if (rc) return rc;
  HOST_SYNC_CHECK(m, st);
  return QCE_OK;
}

}  // namespace

// A host batch host_chunk_rows() cuts into C-row chunks: straight from / into the caller's arrays where both can be
// DMA'd, else staged through pinned slots
int estimate_host_chunked(qce_model* m, const double* y, long long B, long long C, int mode, double mode_param,
                          double* h_out, hipStream_t st) {
  const char* de = getenv("QCE_HOST_DIRECT");  // QCE_HOST_DIRECT=0: the staged pipeline only (A/B runs, tests)
  if (!(de && de[0] == '0')) {
    HostDma dy(const_cast<double*>(y), sizeof(double2) * (size_t)B * m->M);
    HostDma dh(h_out, sizeof(double2) * (size_t)B * m->N);
    if (dy.ok && dh.ok) {
      const int drc = estimate_host_direct(m, y, B, mode, mode_param, h_out, st);
      if (drc != kDirectNoScratch) return drc;
    }
  }
  return estimate_host_pipelined(m, y, B, C, mode, mode_param, h_out, st);
}

extern "C" {

int qce_host_alloc(size_t bytes, void** out) {
  if (!out) return qce_set_error(QCE_EARG, "null argument");
  *out = nullptr;
  HIPCHK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return QCE_OK;
}

int qce_host_free(void* p) {
  if (p) HIPCHK(hipHostFree(p));
  return QCE_OK;
}

}  // extern "C"
