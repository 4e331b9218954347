// Two-pass form of the FP64 3M estimate kernel (included by qce_f64g_kernel.h, which describes the products, the
// block contents and the scheduling).  A workgroup's segment -- a whole tile or a stream-K slice [klo, khi) of one --
// runs its component range twice:
//
//   pass 1 (log-prob): streams the GL blocks of k = klo .. khi - 1.  Nothing of the filter is live, so all KS
//     fragments yr = hs - hd stay in registers.  lp_k = c_k - q goes to the workgroup's scratch row k (lane group 0
//     writes the wave's 16 columns, 128 B), every lane keeps the running exact maximum m.
//   between: lane group g turns the rows klo + g, klo + g + 4, ... into p_k = exp(lp_k - m) in place (p = 0 for
//     lp = -inf, the exp_tab64 clamp as before) and the groups' sums are added: s = sum_k p_k.  One exp per
//     (sample, component), no running maximum, no rescale of the accumulators.
//   pass 2 (filter): streams the GW blocks of k = klo .. khi - 1; p_k of the lane's column is read back one
//     component ahead.  B operands p hs, p hd, p yr, the three accumulator sets and the tile write-out as in the
//     single-pass kernel.
//
// The table is two regions, GL[K] then GW[K] (k_pack_f64g2), each padded to whole ring chunks of one shared size, so
// the LDS ring, its barriers and the refill are those of the single-pass kernel; only the cursor differs: per
// segment the GL chunks of [klo, khi), then its GW chunks.  The scratch is K x 128 doubles per workgroup (128 KB at
// K = 128, written and read back by the same CU within one segment; whether it stays in that XCD's 4 MB L2 beside the
// tables was not measured); a wave reads only what it wrote itself, ordered by s_waitcnt vmcnt(0) between the phases.
#pragma once

// LDS operand prefetch distance (blocks) of the two passes.  Pass 1 has the registers for a deep window: kernel time
// at 8 was 0.5 to 0.8 % below 4 in two sessions, 2 equal to 4; pass 2, beside the 96 accumulator registers, was
// 0.2 % slower at 3 and 4 than at 2 (profiles/f64g_two_pass_ab.jsonl, sub-steps).
#ifndef QCE_F64G2_E1
#define QCE_F64G2_E1 8
#endif
#ifndef QCE_F64G2_E2
#define QCE_F64G2_E2 2
#endif
// 1: ring refills with the chunk's base in SGPRs (lds_dma16's SGPR-base form); 0: a 64-bit VGPR address per piece
#ifndef QCE_F64G_SDMA
#define QCE_F64G_SDMA 1
#endif

namespace {

template <int MP, int NP, bool HM>
struct F64G2 {
  static constexpr int NTL = MP / 16, NTW = NP / 16, KS = MP / 4, KU = KS / 2;
  static constexpr int HMI = HM ? 1 : 0;
  static constexpr __host__ __device__ int gl_units(int T) { return 2 * T + 2; }
  static constexpr int GL_BLOCKS = f64g_gl_blocks(MP, HMI);
  static constexpr int GW_BLOCKS = f64g_gw_blocks(MP, NP, HMI);
  static constexpr int CB = f64g2_cb(GL_BLOCKS, GW_BLOCKS);
  static constexpr int NSLOT = 144 / CB < 8 ? 144 / CB : 8;
  static constexpr int CHUNK = CB * 1024;
  static constexpr int BPC_L = f64g2_bpc_l(MP, NP, HMI), BPC_W = f64g2_bpc_w(MP, NP, HMI);
  static constexpr int CPC_L = BPC_L / CB, CPC_W = BPC_W / CB;
  static_assert(BPC_L % CB == 0 && BPC_W % CB == 0, "whole chunks");
};

// Source cursor of the two-pass ring.  Segments in the kernel's order: R whole tiles (components 0 .. K - 1), then
// the tail items from component c0 on, a new segment wherever the component wraps to 0.  Per segment the GL chunks
// of its components, then the GW chunks.  Past the end it stays on the last chunk (dummy refills, never read).
struct RingCursor2 {
  int rounds, tail_left, tail_next, K, cpc_l, cpc_w;
  int klo, khi, k, cc, pass, done;
  QCE_DEV void next_seg() {
    if (rounds > 0) {
      --rounds;
      klo = 0;
      khi = K;
    } else if (tail_left > 0) {
      klo = tail_next;
      const int n = K - klo < tail_left ? K - klo : tail_left;
      khi = klo + n;
      tail_left -= n;
      tail_next = 0;
    } else {
      done = 1;
      pass = 1;
      k = khi - 1;
      cc = cpc_w - 1;
      return;
    }
    pass = 0;
    k = klo;
    cc = 0;
  }
  QCE_DEV void init(int R, int c0, int ntail, int K_, int cpc_l_, int cpc_w_) {
    rounds = R;
    tail_left = ntail;
    tail_next = c0;
    K = K_;
    cpc_l = cpc_l_;
    cpc_w = cpc_w_;
    klo = 0;
    khi = 1;
    done = 0;
    next_seg();
  }
  QCE_DEV long long chunk_index() const {
    return pass ? (long long)K * cpc_l + (long long)k * cpc_w + cc : (long long)k * cpc_l + cc;
  }
  QCE_DEV void advance() {
    if (done) return;
    if (++cc < (pass ? cpc_w : cpc_l)) return;
    cc = 0;
    if (++k < khi) return;
    if (pass == 0) {
      pass = 1;
      k = klo;
      return;
    }
    next_seg();
  }
};

// Scratch reads go to the L2 (agent-scope load): the row was last written by another lane of the same wave, and an
// older copy of its line may sit in the CU's vector L1 from the previous segment.
QCE_DEV double scr_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace

template <int MP, int NP, bool HM, bool OUT_PARTIAL>
__global__ __launch_bounds__(F64G_NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_est_all_f64g2(
    long long B, int M, int N, int K, int R, long long L, const double2* __restrict__ y, const char* __restrict__ pack,
    const double* __restrict__ cconst, double2* __restrict__ h, double* __restrict__ om, double* __restrict__ os,
    double* __restrict__ oa, double* __restrict__ pm, double* __restrict__ ps, double* __restrict__ pa,
    double* __restrict__ pk, const double* __restrict__ shift, double* pscr, unsigned long long* __restrict__ stamps) {
  using G = F64G2<MP, NP, HM>;
  constexpr int NW = F64G_NW;      // waves of 16 samples, two per SIMD
  constexpr int TS = NW * 16;      // samples per tile
  constexpr int LPW = G::CB / NW;  // global_load_lds pieces per wave per chunk
  constexpr int E1 = QCE_F64G2_E1, E2 = QCE_F64G2_E2;
  static_assert(G::CB % NW == 0, "chunk split");
  static_assert(E1 < G::CB && E2 < G::CB, "the prefetch window must stay inside one chunk");
  static_assert(G::NSLOT >= 3, "ring depth");
  __shared__ __attribute__((aligned(16))) char lds[G::NSLOT * G::CHUNK];
  __shared__ double etab[32];  // 2^(j/32) for exp_tab64

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, col = lane & 15;
  if (threadIdx.x < 32) etab[threadIdx.x] = exp2((double)threadIdx.x / 32.0);  // visible after the first barrier
  const long long P = gridDim.x, w = blockIdx.x;
  const long long tiles = (B + TS - 1) / TS;
  const long long tail0 = (long long)R * P;
  const long long item0 = w * L;
  const long long tail_items = (tiles - tail0) * K;
  const long long item1 = (item0 + L < tail_items) ? item0 + L : tail_items;
  const long long ntail = item1 > item0 ? item1 - item0 : 0;
  if ((long long)R == 0 && ntail == 0) return;  // nothing for this workgroup (uniform)
  const long long t_first = tail0 + (L > 0 ? item0 / K : 0);
  const long long nseg = (long long)R + (ntail > 0 ? (item1 - 1) / K - item0 / K + 1 : 0);

  F64_STAMP_DECL
  // ---- ring (as k_est_all_f64g; the cursor walks GL then GW chunks per segment) ----
  RingCursor2 cur;
  cur.init(R, (int)(item0 % K), (int)ntail, K, G::CPC_L, G::CPC_W);
  int issued = 0;
  const char* rsrc = pack;
  int rdst = 0;
#if QCE_F64G_SDMA
  unsigned rlane = lane * 16;
  asm volatile("" : "+v"(rlane));
  auto refill_begin = [&]() {
    rsrc = uniform_ptr(pack + cur.chunk_index() * (long long)G::CHUNK + wave * 1024);
    rdst = (issued % G::NSLOT) * G::CHUNK + wave * 1024;
    cur.advance();
    ++issued;
  };
  auto refill_pieces = [&](int lo, int hi) {
    for (int i = lo; i < hi; ++i) lds_dma16(rsrc + i * NW * 1024, rlane, lds + rdst + i * NW * 1024);
  };
#else
  auto refill_begin = [&]() {
    rsrc = pack + cur.chunk_index() * (long long)G::CHUNK + wave * 1024 + lane * 16;
    rdst = (issued % G::NSLOT) * G::CHUNK + wave * 1024;
    cur.advance();
    ++issued;
  };
  auto refill_pieces = [&](int lo, int hi) {
    for (int i = lo; i < hi; ++i) lds_dma16(rsrc + i * NW * 1024, lds + rdst + i * NW * 1024);
  };
#endif
  // chunk j lands by barrier j: at barrier j the slot of chunk j - 2 is free and takes chunk j + NSLOT - 2
  auto boundary_wait = [&]() {
    wait_vmcnt<(G::NSLOT - 3) * LPW>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    F64_STAMP(3);
  };
#pragma unroll 1
  for (int j = 0; j < G::NSLOT - 2; ++j) {
    refill_begin();
    refill_pieces(0, LPW);
  }
  boundary_wait();  // chunk 0
  refill_begin();
  refill_pieces(0, LPW);
  int cstream = 0;
  double* const scr = pscr + w * (long long)K * TS + wave * 16 + col;  // row k of the lane's column at scr[k * TS]

  for (long long seg = 0; seg < nseg; ++seg) {
    long long t;
    int klo, khi;
    if (seg < R) {
      t = seg * P + w;
      klo = 0;
      khi = K;
    } else {
      t = tail0 + item0 / K + (seg - R);
      const long long tK = (t - tail0) * K;
      klo = (int)((item0 > tK ? item0 : tK) - tK);
      khi = (int)((tK + K < item1 ? tK + K : item1) - tK);
    }
    const long long sbase = t * TS + (long long)wave * 16;
    // y fragments: k-step s, lane group g -> complex column 4s + g as (hs, hd) = ((yr + yi) / 2, (yi - yr) / 2).
    // Rows past B and columns past M are clamped (finite values meeting zero table entries / never written).
    double2 hv[G::KS];
    {
      int gl = g, cl = col;
      asm volatile("" : "+v"(gl), "+v"(cl));
      long long sm = sbase + cl;
      sm = sm < B ? sm : B - 1;
      const double2* yr = y + sm * M;
#pragma unroll
      for (int s = 0; s < G::KS; ++s) {
        const int cc = 4 * s + gl;
        hv[s] = yr[cc < M ? cc : M - 1];
      }
      wait_vmcnt<0>();
#pragma unroll
      for (int s = 0; s < G::KS; ++s) {
        const double a = hv[s].x, b = hv[s].y;
        hv[s] = make_double2(0.5 * (a + b), 0.5 * (b - a));
      }
    }
    F64_STAMP(5);

    // ---- pass 1: log-probabilities of [klo, khi) into the scratch, exact maximum m ----
    double m = QCE_NEG_INF;
    {
      double yrv[G::KS];
#pragma unroll
      for (int s = 0; s < G::KS; ++s) yrv[s] = hv[s].x - hv[s].y;
#pragma unroll 1
      for (int k = klo; k < khi; ++k) {
        const double ck = cconst[k];
        int rslot = cstream % G::NSLOT;
        int roff = lane * 16 + rslot * G::CHUNK;
        auto rd = [&](int off) -> double2 { return *reinterpret_cast<const double2*>(&lds[roff + off]); };
        f64x4 k1 = f64x4{0.0, 0.0, 0.0, 0.0}, rr = k1, ii = k1;
        double qp = 0.0;
        double2 buf[E1 + 1];
#pragma unroll
        for (int i = 0; i < E1; ++i) buf[i] = rd(i * 1024);
        static_for(
            [&](auto bc) {
              constexpr int b = decltype(bc)::value;
              constexpr BlockInfo3 bi = block_info3_pass(MP, NP, G::HMI, 0, b);
              __builtin_amdgcn_sched_barrier(0);
              constexpr bool RB = (b + E1) % G::CB == 0;
              if constexpr (RB) {
                F64_STAMP(0);
                boundary_wait();
                refill_begin();
              }
              if constexpr (b + E1 < G::BPC_L) {
                constexpr int r = b + E1;
                if constexpr (r % G::CB == 0) {
                  rslot = rslot + 1 == G::NSLOT ? 0 : rslot + 1;
                  roff = lane * 16 + rslot * G::CHUNK;
                  asm volatile("" : "+v"(roff));
                }
                buf[r % (E1 + 1)] = rd((r % G::CB) * 1024);
              }
              const double2 a = buf[b % (E1 + 1)];
              constexpr int NMF = bi.kind == 4 ? 0 : 2;
              int jm = 0;
              auto gap = [&]() {
                if constexpr (RB && NMF > 0) {
                  __builtin_amdgcn_sched_barrier(0);
                  refill_pieces(jm * LPW / NMF, (jm + 1) * LPW / NMF);
                  __builtin_amdgcn_sched_barrier(0);
                }
                ++jm;
              };
              constexpr int s0 = 2 * bi.u, s1 = 2 * bi.u + 1;
              if constexpr (bi.kind == 0) {  // GL data
                if constexpr (bi.j == 0) {
                  k1 = mfma16x16x4d(a.x, yrv[s0], k1);
                  gap();
                  rr = mfma16x16x4d(a.y, hv[s0].x, rr);
                  gap();
                } else if constexpr (bi.j == 1) {
                  ii = mfma16x16x4d(a.x, hv[s0].y, ii);
                  gap();
                  k1 = mfma16x16x4d(a.y, yrv[s1], k1);
                  gap();
                } else {
                  rr = mfma16x16x4d(a.x, hv[s1].x, rr);
                  gap();
                  ii = mfma16x16x4d(a.y, hv[s1].y, ii);
                  gap();
                }
              } else if constexpr (bi.kind == 1) {  // GL mean column (-q0): B = 1 in lane group 0
                const double one = g == 0 ? 1.0 : 0.0;
                rr = mfma16x16x4d(a.x, one, rr);
                gap();
                ii = mfma16x16x4d(a.y, one, ii);
                gap();
              }
              if constexpr (RB && NMF == 0) refill_pieces(0, LPW);
              // end of a GL row tile: |z|^2 of its 16 complex rows into the lane's quad-form partial
              if constexpr (bi.kind == 0 || bi.kind == 1) {
                constexpr bool last = HM ? (bi.kind == 1) : (bi.u == G::gl_units(bi.T) - 1 && bi.j == 2);
                if constexpr (last) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) {
                    const double zr = k1[i] + rr[i], zi = k1[i] + ii[i];
                    qp = fma(zr, zr, qp);
                    qp = fma(zi, zi, qp);
                  }
                  asm volatile("" : "+v"(qp));
                  k1 = rr = ii = f64x4{0.0, 0.0, 0.0, 0.0};
                }
              }
              if constexpr (b == G::GL_BLOCKS - 1) {  // after the last GL block: the log-probability
                const double lp = ck - sum_groups(qp);
                m = fmax(m, lp);
                if (g == 0) scr[(long long)k * TS] = lp;
              }
            },
            std::make_integer_sequence<int, G::BPC_L>{});
        F64_STAMP(0);
        cstream += G::CPC_L;
      }
    }

    // ---- between the passes: p_k = exp(lp_k - m) in place, lane group g the rows klo + g + 4 j; s = sum_k p_k ----
    double ssum = 0.0;
    wait_vmcnt<0>();  // this wave's lp stores (drains the ring's refills too: once per segment)
    {
      int gs = g;
      asm volatile("" : "+v"(gs));
#pragma unroll 1
      for (int k = klo + gs; k < khi; k += 16) {  // four rows per trip: their loads in flight together
        double lp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) lp[j] = k + 4 * j < khi ? scr_load(scr + (long long)(k + 4 * j) * TS) : QCE_NEG_INF;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + 4 * j < khi) {
            const double p = (lp[j] == QCE_NEG_INF) ? 0.0 : exp_tab64(lp[j] - m, etab);
            scr[(long long)(k + 4 * j) * TS] = p;
            ssum += p;
          }
      }
      ssum = sum_groups(ssum);
    }
    wait_vmcnt<0>();  // the p stores, before other lanes of the wave read them
    F64_STAMP(1);

    // ---- pass 2: the filter sums over [klo, khi) ----
    f64x4 ok[G::NTW], orr[G::NTW], oi[G::NTW];
#pragma unroll
    for (int T = 0; T < G::NTW; ++T) ok[T] = orr[T] = oi[T] = f64x4{0.0, 0.0, 0.0, 0.0};
    double pn = scr_load(scr + (long long)klo * TS);
    asm volatile("" : "+v"(pn));  // landed before the loop: its wait is not repeated per component
#pragma unroll 1
    for (int k = klo; k < khi; ++k) {
      const double p = pn;
      // p of the next component: issued now, first touched after this component's first ring barrier.  The compiler
      // waits for it with s_waitcnt vmcnt(0), one per component, which also waits for the newest refill in flight
      // (issued one chunk of MFMAs earlier) one barrier sooner than the ring itself would: expected to be landed by
      // then, not measured apart from the kernel's time.
      pn = scr_load(scr + (long long)(k + 1 < khi ? k + 1 : k) * TS);
      int rslot = cstream % G::NSLOT;
      int roff = lane * 16 + rslot * G::CHUNK;
      auto rd = [&](int off) -> double2 { return *reinterpret_cast<const double2*>(&lds[roff + off]); };
      double pr0 = 0.0, ps0 = 0.0, pd0 = 0.0, pr1 = 0.0, ps1 = 0.0, pd1 = 0.0;
      double2 buf[E2 + 1];
#pragma unroll
      for (int i = 0; i < E2; ++i) buf[i] = rd(i * 1024);
      static_for(
          [&](auto bc) {
            constexpr int b = decltype(bc)::value;
            constexpr BlockInfo3 bi = block_info3_pass(MP, NP, G::HMI, 1, b);
            __builtin_amdgcn_sched_barrier(0);
            constexpr bool RB = (b + E2) % G::CB == 0;
            if constexpr (RB) {
              F64_STAMP(2);
              boundary_wait();
              if constexpr (b == G::CB - E2) asm volatile("" : "+v"(pn));
              refill_begin();
            }
            if constexpr (b + E2 < G::BPC_W) {
              constexpr int r = b + E2;
              if constexpr (r % G::CB == 0) {
                rslot = rslot + 1 == G::NSLOT ? 0 : rslot + 1;
                roff = lane * 16 + rslot * G::CHUNK;
                asm volatile("" : "+v"(roff));
              }
              buf[r % (E2 + 1)] = rd((r % G::CB) * 1024);
            }
            const double2 a = buf[b % (E2 + 1)];
            constexpr int NMF = bi.kind == 4 ? 0 : 2;
            int jm = 0;
            auto gap = [&]() {
              if constexpr (RB && NMF > 0) {
                __builtin_amdgcn_sched_barrier(0);
                refill_pieces(jm * LPW / NMF, (jm + 1) * LPW / NMF);
                __builtin_amdgcn_sched_barrier(0);
              }
              ++jm;
            };
            constexpr int s0 = 2 * bi.u, s1 = 2 * bi.u + 1;
            if constexpr (bi.kind == 2) {  // GW data: B operands formed once per component, j phase by j phase
              if constexpr (bi.T == 0 && bi.j == 0) {
                ps0 = p * hv[s0].x;
                pd0 = p * hv[s0].y;
                pr0 = ps0 - pd0;
              } else if constexpr (bi.T == 0 && bi.j == 1) {
                ps1 = p * hv[s1].x;
                pd1 = p * hv[s1].y;
                pr1 = ps1 - pd1;
              }
              if constexpr (bi.j == 0) {
                ok[bi.T] = mfma16x16x4d(a.x, pr0, ok[bi.T]);
                gap();
                orr[bi.T] = mfma16x16x4d(a.y, ps0, orr[bi.T]);
                gap();
              } else if constexpr (bi.j == 1) {
                oi[bi.T] = mfma16x16x4d(a.x, pd0, oi[bi.T]);
                gap();
                ok[bi.T] = mfma16x16x4d(a.y, pr1, ok[bi.T]);
                gap();
              } else {
                orr[bi.T] = mfma16x16x4d(a.x, ps1, orr[bi.T]);
                gap();
                oi[bi.T] = mfma16x16x4d(a.y, pd1, oi[bi.T]);
                gap();
              }
            } else if constexpr (bi.kind == 3) {  // GW bias column (b): B = p in lane group 0
              const double pone = g == 0 ? p : 0.0;
              orr[bi.T] = mfma16x16x4d(a.x, pone, orr[bi.T]);
              gap();
              oi[bi.T] = mfma16x16x4d(a.y, pone, oi[bi.T]);
              gap();
            }
            if constexpr (RB && NMF == 0) refill_pieces(0, LPW);
          },
          std::make_integer_sequence<int, G::BPC_W>{});
      F64_STAMP(2);
      cstream += G::CPC_W;
    }

    // ---- write the tile: row 16 T + g + 4 i of sample col = (K1 + R', K1 + I') ----
    {
      int gw = g;
      asm volatile("" : "+v"(gw));
      const int ls = wave * 16 + col;
      const long long sample = t * TS + ls;
      if (sample < B) {
        const bool whole = (klo == 0 && khi == K);
        const bool pfmt = OUT_PARTIAL || !whole;
        const long long row = whole ? sample : (w * 2 + (t == t_first ? 0 : 1)) * TS + ls;
        if (OUT_PARTIAL && whole && pk) {  // shifted packed partial: [s e^{m-M*}, 0, acc e^{m-M*}] (K-shard sum)
          const double sc = (m == QCE_NEG_INF) ? 0.0 : exp(m - *shift);
          double* dp = pk + sample * (2LL * N + 2);
          if (g == 0) *reinterpret_cast<double2*>(dp) = make_double2(ssum * sc, 0.0);
#pragma unroll
          for (int T = 0; T < G::NTW; ++T)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int n = 16 * T + gw + 4 * i;
              if (n < N)
                *reinterpret_cast<double2*>(dp + 2 + 2 * n) =
                    make_double2((ok[T][i] + orr[T][i]) * sc, (ok[T][i] + oi[T][i]) * sc);
            }
        } else if (pfmt) {
          double* dm = whole ? om : pm;
          double* ds = whole ? os : ps;
          double* da = (whole ? oa : pa) + row * (2LL * N);
          if (g == 0) {
            dm[row] = m;
            ds[row] = ssum;
          }
#pragma unroll
          for (int T = 0; T < G::NTW; ++T)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int n = 16 * T + gw + 4 * i;
              if (n < N)
                *reinterpret_cast<double2*>(da + 2 * n) = make_double2(ok[T][i] + orr[T][i], ok[T][i] + oi[T][i]);
            }
        } else {
          const double inv = 1.0 / ssum;
          double2* hp = h + sample * N;
#pragma unroll
          for (int T = 0; T < G::NTW; ++T)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int n = 16 * T + gw + 4 * i;
              if (n < N) hp[n] = make_double2((ok[T][i] + orr[T][i]) * inv, (ok[T][i] + oi[T][i]) * inv);
            }
        }
      }
    }
  }
  F64_STAMP(5);
  F64_STAMP_FLUSH
  wait_vmcnt<0>();  // drain the (dummy) ring prefetches before the workgroup retires
}
