// Body of cm_conv_kernel / cm_conv_f16_kernel / cm_conv_h_kernel (comodgan_kernels.hpp, where the template parameters are
// described): included inside the three kernel templates, which define F16 (false: error-compensated fp16 pairs, three MFMAs per
// product; true: the single-plane form, one MFMA per product) and the element types of the activation tensors, XH (p.x holds
// _Float16) and YH (p.y and p.skip hold _Float16); both false in the first two kernels.  `p` is the kernel's CmConvArgs.
  MIGAN_DYN_SMEM(smem);
  constexpr int MT = 64 * MTI, GW = 16, GH = MT / GW, WROWS = 32 * MTI;
  constexpr int WCOLS = NT / 2, NTI = WCOLS / 32;
  constexpr int GS = NT + 4;
  constexpr int RB = KC * 2;                                  // bytes of one plane of one row
  constexpr int NP = F16 ? 1 : 2;                             // fp16 planes per operand
  constexpr int NPR = F16 ? 1 : 3;                            // MFMAs per product
  constexpr int PB = NP * RB + 16;                            // LDS row pitch in bytes (the planes + pad)
  constexpr int NSLOT = KC / 8, QK = KC / 4;                  // 16-byte slots / float4 quads per row and plane
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;

  // logical tile: Cout chunk fastest, then x, y, image (XCD-contiguous ranges share halo rows and weight tiles in L2)
  int t = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int nc = t % p.nchunks; t /= p.nchunks;
  const int tx = t % p.tiles_x; t /= p.tiles_x;
  const int ty = t % p.tiles_y; t /= p.tiles_y;
  const int b = t;
  const int co0 = nc * NT;
  const int gy0 = ty * GH, gx0 = tx * GW;
  const int iy0 = gy0 * p.stride + p.dymin, ix0 = gx0 * p.stride + p.dxmin;
  const int npix = p.IH * p.IW;
  const int nck = p.CI / KC;

  char* a_s = reinterpret_cast<char*>(smem);                  // [npix][PB]
  char* b_s = reinterpret_cast<char*>(smem) + p.off_b;        // [2 buffers][NT][PB]
  float* g_s = smem;                                          // [64][GS] per epilogue pass, after the K loop
  constexpr int b_buf = NT * PB;

  const float* __restrict__ xb = p.x + (size_t)b * p.H * p.W * p.CI;
  // fp16 storage: the same tensor, two bytes per element (the pointers of CmConvArgs are reinterpreted)
  [[maybe_unused]] const unsigned short* __restrict__ xbh = reinterpret_cast<const unsigned short*>(p.x) + (size_t)b * p.H * p.W * p.CI;
  const float* __restrict__ sab = p.sa ? p.sa + (size_t)b * p.CI : nullptr;
  const unsigned w_plane_bytes = (unsigned)(9 * p.CI * p.CO) * 2u;     // bytes of one weight plane (< 2^23)
  [[maybe_unused]] const int total = nck * p.ntaps;            // generic tap list only

  constexpr int NPH = UP4 ? 4 : 1;                            // accumulator sets (output phases)
  static_assert(!UP4 || NINE, "the four-phase mode runs the nine-tap K loop");
  f16v acc[NPH][MTI][NTI];
#pragma unroll
  for (int ph = 0; ph < NPH; ++ph)
#pragma unroll
    for (int i = 0; i < MTI; ++i)
#pragma unroll
      for (int j = 0; j < NTI; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ph][i][j][r] = 0.0f;
  // phase profile (MIGAN_PHASE_PROF builds): 0 prologue, 1 load issue, 2 LDS reads + MFMAs, 3 weight tile -> LDS (incl. the wait for
  // its loads), 4 barrier, 5 input tile -> LDS + barrier, 6 epilogue
  PROF_BEGIN();

  // ---- input-tile items of this thread: item = tid + k*256 -> pixel q = item / QK, channel quad c4 = item % QK
  // (c4 is the same for every k).  goff = element offset of the pixel's channel 0 in the image, -1 = zero padding / no item.
  const int c4 = tid & (QK - 1);
  int goff[NIA];
#pragma unroll
  for (int k = 0; k < NIA; ++k) {
    const int q = (tid + k * 256) / QK;
    const int py = q / p.IW, px = q - py * p.IW;
    const int iy = iy0 + py, ix = ix0 + px;
    goff[k] = (q < npix && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) ? (iy * p.W + ix) * p.CI + c4 * 4 : -1;
  }
  // XH: an item is four halves, one 8-byte load; the prefetch registers keep the raw halves (half the registers) and store_a
  // widens them, so the conversions sit in the staging step with the scaling, outside the tap loop
  typename Io<XH ? 2 : 0>::raw4 areg[NIA];
  auto load_a = [&](int c) {
#pragma unroll
    for (int k = 0; k < NIA; ++k) {
      if constexpr (XH) {
        areg[k] = u2v{0u, 0u};
        if (goff[k] >= 0) areg[k] = *reinterpret_cast<const u2v*>(xbh + (size_t)(unsigned)goff[k] + c * KC);
      } else {
        areg[k] = f4{0.f, 0.f, 0.f, 0.f};
        if (goff[k] >= 0) areg[k] = ld4(xb + (size_t)(unsigned)goff[k] + c * KC);
      }
    }
  };
  auto store_a = [&](int c) {
    f4 sc = f4{p.a_scale, p.a_scale, p.a_scale, p.a_scale};
    if (sab) sc = ld4(sab + c * KC + c4 * 4);
#pragma unroll
    for (int k = 0; k < NIA; ++k) {
      const int q = (tid + k * 256) / QK;
      if (q < npix) {
        u2v h1, h2;
        split2_f16(Io<XH ? 2 : 0>::cvt(areg[k]) * sc, h1, h2);
        char* dst = a_s + q * PB + c4 * 8;
        *reinterpret_cast<u2v*>(dst) = h1;
        if constexpr (!F16) *reinterpret_cast<u2v*>(dst + RB) = h2;
      }
    }
  };

  // ---- weight tile of (tap plane wt, channel chunk c): rows co0..co0+NT-1 of [tap][CI/32][CO][32], both planes.
  // Per-thread pieces (16 bytes each): the lane byte offset inside the tile and the LDS destination are constants of the
  // thread; the tile's base address is wave-uniform (SGPR pair + 32-bit lane offset: no 64-bit VALU address adds).
  constexpr int BTOTAL = NP * NT * NSLOT;                     // 16-byte pieces of a tile
  constexpr int BPIECES = BTOTAL >= 256 ? BTOTAL / 256 : 1;   // per thread
  // (the single-plane 64-column tile of 16-channel chunks has 128 pieces: the first two waves carry one each)
  constexpr bool BPART = BTOTAL < 256;
  static_assert(BPART ? (BTOTAL % 64 == 0) : (BTOTAL % 256 == 0), "weight-tile pieces: whole waves");
  const bool b_on = !BPART || tid < BTOTAL;                   // wave-uniform
  unsigned bsrc[BPIECES];
  int bdst[BPIECES];
#pragma unroll
  for (int k = 0; k < BPIECES; ++k) {
    const int piece = tid + k * 256;                          // [plane][row][slot]
    const int pl = piece / (NT * NSLOT), rs = piece % (NT * NSLOT);
    const int row = rs / NSLOT, slot = rs % NSLOT;
    bsrc[k] = (unsigned)pl * w_plane_bytes + (unsigned)(row * 64 + slot * 16);
    bdst[k] = row * PB + pl * RB + slot * 16;
  }
  f4 breg[2][BPIECES];                                        // two register sets: the NINE path keeps two tiles in flight
  auto load_b = [&](int c, int tp, auto set) {
    constexpr int S = decltype(set)::value;
    const int c32 = (c * KC) >> 5, hc = ((c * KC) & 31) >> 3;  // 32-channel chunk of the planes, first 16-byte slot inside it
    const float* src = reinterpret_cast<const float*>(p.wsplit + ((size_t)(p.wtap[tp] * (p.CI >> 5) + c32) * p.CO + co0) * 32 + hc * 8);
#pragma unroll
    for (int k = 0; k < BPIECES; ++k) {
      if constexpr (BPART) { if (b_on) breg[S][k] = ld4(at_bytes(src, bsrc[k])); }
      else breg[S][k] = ld4(at_bytes(src, bsrc[k]));
    }
  };
  auto store_b = [&](int buf, auto set) {
    constexpr int S = decltype(set)::value;
#pragma unroll
    for (int k = 0; k < BPIECES; ++k) {
      if constexpr (BPART) { if (b_on) st4(reinterpret_cast<float*>(b_s + buf * b_buf + bdst[k]), breg[S][k]); }
      else st4(reinterpret_cast<float*>(b_s + buf * b_buf + bdst[k]), breg[S][k]);
    }
  };
  // ---- MFMA operand addresses: lane (l31, half) supplies row l31 of a 32-row tile, k = 8 * half .. + 7 of a 16-k step
  int a_off[MTI], b_off[NTI];
#pragma unroll
  for (int i = 0; i < MTI; ++i) {
    const int m = cm_pixel_of_row(wm * WROWS + i * 32 + l31);
    a_off[i] = (((m >> 4) * p.stride) * p.IW + (m & 15) * p.stride) * PB + half * 16;
  }
#pragma unroll
  for (int j = 0; j < NTI; ++j) b_off[j] = (wn * WCOLS + j * 32 + l31) * PB + half * 16;
  // MFMAs of one filter tap: A rows = the staged input tile shifted by the tap's offset, B = weight tile in LDS buffer `buf`
  auto mfma_tap = [&](int tp, int buf, auto phc) {
    constexpr int PH = decltype(phc)::value;                   // accumulator set of this tap
    const int delta = ((p.dy[tp] - p.dymin) * p.IW + (p.dx[tp] - p.dxmin)) * PB;       // wave-uniform
    const char* aa[MTI];
    const char* bb[NTI];
#pragma unroll
    for (int i = 0; i < MTI; ++i) aa[i] = a_s + (a_off[i] + delta);
#pragma unroll
    for (int j = 0; j < NTI; ++j) bb[j] = b_s + (b_off[j] + buf * b_buf);
#pragma unroll
    for (int ks = 0; ks < KC / 16; ++ks) {
      f4 av[MTI][NP], bv[NTI][NP];
#pragma unroll
      for (int i = 0; i < MTI; ++i) {
        av[i][0] = ld4(reinterpret_cast<const float*>(aa[i] + ks * 32));
        if constexpr (!F16) av[i][1] = ld4(reinterpret_cast<const float*>(aa[i] + ks * 32 + RB));
      }
#pragma unroll
      for (int j = 0; j < NTI; ++j) {
        bv[j][0] = ld4(reinterpret_cast<const float*>(bb[j] + ks * 32));
        if constexpr (!F16) bv[j][1] = ld4(reinterpret_cast<const float*>(bb[j] + ks * 32 + RB));
      }
      // product-major order: consecutive MFMAs write different accumulators (a dependent MFMA issued straight after
      // its producer waits out the 16-pass latency), smallest products first
#pragma unroll
      for (int pr = 0; pr < NPR; ++pr)
#pragma unroll
        for (int i = 0; i < MTI; ++i)
#pragma unroll
          for (int j = 0; j < NTI; ++j)
            acc[PH][i][j] = MIGAN_MFMA_F16_32X32X16(av[i][(!F16 && pr == 0) ? 1 : 0], bv[j][(!F16 && pr == 1) ? 1 : 0], acc[PH][i][j]);
    }
  };

  if constexpr (!NINE) {
    // ---- generic tap list (the 1/2/4-tap phases of the transposed convolution): weight tile prefetched one tap ahead.
    // One filter tap of channel chunk c: issue the next weight tile's loads (and, on the last tap of the chunk, the next
    // chunk's input-tile loads: they fly under this tap's MFMAs and are consumed by store_a right after the barrier),
    // MFMAs of this tap from LDS, next weight tile -> LDS, barrier.  The prefetches are unconditional (the last ones
    // re-load the last tile) so that no branch sits between a load and its use.
    auto tap_body = [&](int c, int tp, auto prefetch_a) {
      const int it = c * p.ntaps + tp;
      int cn = c, tn = tp + 1;
      if (tn == p.ntaps) { tn = 0; ++cn; }
      if (cn == nck) { cn = c; tn = tp; }
      load_b(cn, tn, IntT<0>{});
      if constexpr (decltype(prefetch_a)::value) load_a(c + 1 < nck ? c + 1 : c);
      if constexpr (MTI == 2 && !decltype(prefetch_a)::value) {
        // same pipeline hints as the nine-tap path: operand reads, weight loads spread over the first step's MFMAs
        mfma_tap(tp, it & 1, IntT<0>{});
        constexpr int M = MTI * NTI * NPR, RD = (MTI + NTI) * NP;
        constexpr int A1 = M / BPIECES > 0 ? M / BPIECES : 1;
        MIGAN_SCHED_GROUP(0x100, RD);
#pragma unroll
        for (int k = 0; k < BPIECES; ++k) {
          MIGAN_SCHED_GROUP(0x008, A1);
          MIGAN_SCHED_GROUP(0x020, 1);
        }
        if constexpr (M - A1 * BPIECES > 0) MIGAN_SCHED_GROUP(0x008, M - A1 * BPIECES);
        MIGAN_SCHED_GROUP(0x100, RD);
        MIGAN_SCHED_GROUP(0x008, M);
      } else {
        MIGAN_SCHED_FENCE();        // keep the loads ahead of the MFMAs (the scheduler otherwise sinks them to their use)
        mfma_tap(tp, it & 1, IntT<0>{});
      }
      MIGAN_SCHED_FENCE();
      store_b((it + 1) & 1, IntT<0>{});
      __syncthreads();
    };
    load_a(0);
    load_b(0, 0, IntT<0>{});
    store_b(0, IntT<0>{});
    for (int c = 0; c < nck; ++c) {
      // input halo tile of channel chunk c: registers -> x style scale -> two fp16 planes in LDS
      store_a(c);
      __syncthreads();
      for (int tp = 0; tp + 1 < p.ntaps; ++tp) tap_body(c, tp, FalseT{});
      tap_body(c, p.ntaps - 1, TrueT{});
    }
  } else {
    // ---- nine taps (plain and strided 3x3): two weight tiles are kept in flight in two register sets.  The K loop is
    // straight-line code over two channel chunks (18 taps: the register set of a tile is its global tap index mod 2, a
    // compile-time constant), which also lets the compiler count outstanding loads exactly (no s_waitcnt vmcnt(0) at
    // control-flow joins).
    //   tap `it`:  issue loads of tile it+2 -> set it%2 | MFMAs of tap it from LDS buffer it%2 |
    //              tile it+1 (set (it+1)%2, in flight since tap it-1) -> LDS buffer (it+1)%2 | barrier
    // The next chunk's input tile is loaded two taps before the chunk ends, ahead of that tap's weight loads, so waiting
    // for it at the chunk boundary leaves the newer weight loads in flight.
    auto tap9 = [&](int c, auto tpc, auto parc) {
      constexpr int TP = decltype(tpc)::value, PAR = decltype(parc)::value;
      constexpr int TN = (TP + 2) % 9, CN = (TP + 2) / 9;      // tile two taps ahead
      if constexpr (TP == 7) load_a(c + 1 < nck ? c + 1 : c);
      const bool inside = c + CN < nck;                        // beyond the end: re-load the last tile (never used)
      load_b(inside ? c + CN : nck - 1, inside ? TN : 8, IntT<PAR>{});
      if constexpr (MTI == 2) {
        // Two-waves-per-SIMD tiles: instruction-class pipeline hints instead of hard fences (phase profile: 30 % of a tap went
        // to issuing the weight loads, storing the previous tile to LDS and the barrier, serialised around the MFMAs): first
        // 16-k step's operand reads, the weight-tile loads spread over its MFMAs, then the second step.  Measured +8..12 % on
        // the 64- and 128-column kernels; the 512-register 16 x 16 tiles lose 5 % with it and keep the fences.
        mfma_tap(TP, PAR, IntT<(UP4 ? (((TP / 3) == 1) * 2 + ((TP % 3) == 1)) : 0)>{});
        store_b(PAR ^ 1, IntT<PAR ^ 1>{});
        constexpr int M = MTI * NTI * NPR, RD = (MTI + NTI) * NP, NKS = KC / 16;
        constexpr int A1 = M / BPIECES > 0 ? M / BPIECES : 1;
        MIGAN_SCHED_GROUP(0x100, RD);
#pragma unroll
        for (int k = 0; k < BPIECES; ++k) {
          MIGAN_SCHED_GROUP(0x008, A1);
          MIGAN_SCHED_GROUP(0x020, 1);
        }
        if constexpr (M - A1 * BPIECES > 0) MIGAN_SCHED_GROUP(0x008, M - A1 * BPIECES);
        if constexpr (NKS == 2) {
          MIGAN_SCHED_GROUP(0x100, RD);
#pragma unroll
          for (int k = 0; k < BPIECES; ++k) {
            MIGAN_SCHED_GROUP(0x008, A1);
            MIGAN_SCHED_GROUP(0x200, 1);
          }
          if constexpr (M - A1 * BPIECES > 0) MIGAN_SCHED_GROUP(0x008, M - A1 * BPIECES);
        } else {
          MIGAN_SCHED_GROUP(0x200, BPIECES);
        }
        __syncthreads();
      } else {
        MIGAN_SCHED_FENCE();
        PROF_MARK(1);
        mfma_tap(TP, PAR, IntT<(UP4 ? (((TP / 3) == 1) * 2 + ((TP % 3) == 1)) : 0)>{});
        MIGAN_SCHED_FENCE();
        PROF_MARK(2);
        store_b(PAR ^ 1, IntT<PAR ^ 1>{});
        PROF_MARK(3);
        __syncthreads();
        PROF_MARK(4);
      }
    };
    auto chunk9 = [&](int c, auto cpar) {
      constexpr int CP = decltype(cpar)::value;         // parity of the chunk's first global tap index
      store_a(c);
      __syncthreads();
      PROF_MARK(5);
      tap9(c, IntT<0>{}, IntT<CP>{});     tap9(c, IntT<1>{}, IntT<CP ^ 1>{}); tap9(c, IntT<2>{}, IntT<CP>{});
      tap9(c, IntT<3>{}, IntT<CP ^ 1>{}); tap9(c, IntT<4>{}, IntT<CP>{});     tap9(c, IntT<5>{}, IntT<CP ^ 1>{});
      tap9(c, IntT<6>{}, IntT<CP>{});     tap9(c, IntT<7>{}, IntT<CP ^ 1>{}); tap9(c, IntT<8>{}, IntT<CP>{});
    };
    load_a(0);
    load_b(0, 0, IntT<0>{});
    load_b(0, 1, IntT<1>{});
    store_b(0, IntT<0>{});
    PROF_MARK(0);
    for (int c = 0; c < nck; c += 2) {      // nck is even (host check)
      chunk9(c, IntT<0>{});
      chunk9(c + 1, IntT<1>{});
    }
  }

  // ---- epilogue, one pass per MFMA row tile i (64 GEMM rows: rows i*32..i*32+31 of both wave rows): accumulators -> LDS result
  // tile -> per float4: coefficient, noise, bias, activation, skip
  const float inv_wscale = 1.0f / reinterpret_cast<const float*>(p.wsplit)[-2];      // power of two (cm_split_conv_kernel)
  const float ns = p.noise ? p.noise_strength[0] : 0.0f;
  constexpr int QN = NT / 4;
  static_assert(256 % QN == 0 && (64 * QN) % 256 == 0, "epilogue items: one channel quad per thread");
  const int eq_q4 = tid % QN, eq_row = tid / QN, eq_co = co0 + eq_q4 * 4;
  const f4 eq_cf = (p.coef ? ld4(p.coef + (size_t)b * p.CO + eq_co) : f4{p.cgain, p.cgain, p.cgain, p.cgain}) * inv_wscale;
  const bool raw_out = UP4 || p.raw != 0;                      // (the four-phase launch always writes the raw tensor: cm_fir_kernel<1> finishes the layer)
  const f4 eq_bias = raw_out ? f4{0.f, 0.f, 0.f, 0.f} : ld4(p.bias + eq_co);
#pragma unroll
  for (int ph = 0; ph < NPH; ++ph) {
    // four-phase mode: phase (ey, ex) writes raw[2 g + e]; its grid extent is H + (ey == 0) by W + (ex == 0)
    const int ey = ph >> 1, ex = ph & 1;
    const int ghn = UP4 ? p.H + (ey == 0) : p.GHn, gwn = UP4 ? p.W + (ex == 0) : p.GWn;
    const int oym = UP4 ? 2 : p.oy_mul, oya = UP4 ? ey : p.oy_add, oxm = UP4 ? 2 : p.ox_mul, oxa = UP4 ? ex : p.ox_add;
#pragma unroll
    for (int i = 0; i < MTI; ++i) {
      if (ph + i > 0) __syncthreads();       // the previous pass has been read (first pass: the K loop ended with a barrier)
#pragma unroll
      for (int j = 0; j < NTI; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lrow = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const int col = wn * WCOLS + j * 32 + l31;
          g_s[lrow * GS + col] = acc[ph][i][j][r];
        }
      __syncthreads();
      // a thread's items of a pass share the channel quad (256 % QN == 0): coefficient and bias are read once per workgroup (above);
      // the per-pixel operands (noise, skip) of FOUR items are requested before the first of them is finished and stored -- a load
      // consumed right behind the previous item's store made every item wait for that store (vmcnt retires in order)
      constexpr int IPT = 64 * QN / 256, GRP = UP4 ? 2 : (IPT < 4 ? IPT : 4);       // (the four-phase form sits at its 256-register cap: two items ahead there)
#pragma unroll
      for (int k0 = 0; k0 < IPT; k0 += GRP) {
        size_t o[GRP];
        bool ok[GRP];
        float nz[GRP];
        f4 sk[GRP];
#pragma unroll
        for (int g = 0; g < GRP; ++g) {
          const int lrow = eq_row + (k0 + g) * (256 / QN);
          const int m = cm_pixel_of_row((lrow >> 5) * WROWS + i * 32 + (lrow & 31));
          const int gy = gy0 + (m >> 4), gx = gx0 + (m & 15);
          ok[g] = gy < ghn && gx < gwn;
          const int oy = gy * oym + oya, ox = gx * oxm + oxa;
          o[g] = ok[g] ? (((size_t)b * p.HO + oy) * p.WO + ox) * p.CO + eq_co : 0;
          nz[g] = 0.0f;
          sk[g] = f4{0.f, 0.f, 0.f, 0.f};
          if (!raw_out && ok[g]) {
            if (p.noise) nz[g] = p.noise[(size_t)b * p.noise_bstride + (size_t)oy * p.WO + ox];
            if constexpr (YH) {
              if (p.skip) sk[g] = Io<2>::cvt(MIGAN_LOAD_NT(reinterpret_cast<const u2v*>(reinterpret_cast<const unsigned short*>(p.skip) + o[g])));
            } else {
              if (p.skip) sk[g] = ld4once(p.skip + o[g]);
            }
          }
        }
#pragma unroll
        for (int g = 0; g < GRP; ++g) {
          if (!ok[g]) continue;
          const int lrow = eq_row + (k0 + g) * (256 / QN);
          f4 v = ld4(g_s + lrow * GS + eq_q4 * 4) * eq_cf;
          if (!raw_out) {
            if (p.noise) v = v + MIGAN_FMUL_RN(nz[g], ns);
            v = act4(v + eq_bias);
            if (p.skip) v = v + sk[g];
          }
          // YH: four halves, rounded to nearest even, one 8-byte store
          if constexpr (YH) MIGAN_STORE_NT(reinterpret_cast<u2v*>(reinterpret_cast<unsigned short*>(p.y) + o[g]), (u2v{MIGAN_PACK_F16(v.x, v.y), MIGAN_PACK_F16(v.z, v.w)}));
          else st4o(p.y + o[g], v);
        }
      }
    }
  }
  PROF_MARK(6);
  PROF_END();
