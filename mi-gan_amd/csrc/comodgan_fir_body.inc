// Body of cm_fir_kernel<EPI>, cm_fir_samples_kernel, cm_fir_h_kernel and cm_fir_samples_h_kernel (comodgan_kernels.hpp): the one
// text of the 2 x 4-block [1,3,3,1] FIR.  Included into each kernel like comodgan_conv_body.inc, so that every symbol is compiled
// from its own by-value argument.  The enclosing kernel supplies
//   p                    its CmFirArgs
//   EPI                  0: FIR only; 1: + noise, bias, activation, skip
//   SAMP, S              an S-samples forward: x, y and the noise are per sample ([B = N * S], image-major), the skip tensor is the
//                        encoder's, per image: sample b reads the skip pixels of image b / S.  The flat index carries the sample
//                        right above the channel quad -- (image, block row, block column, sample, quad) -- so the S samples of an
//                        image that share a 2 x 4 block of skip pixels sit in adjacent lane groups of one workgroup or of two
//                        consecutive ones: the first brings the pixels in, the others find them in the vector cache or in L2
//   XH, YH, SH           which of x, y and the skip tensor hold _Float16 (CmAct)
// Arithmetic is fp32 on converted values (the FIR gain included), one rounding, to nearest even, when an fp16 y is written.
  constexpr bool TYPED = XH || YH || SH;
  using XT = CmAct<TYPED, XH>;
  using YT = CmAct<TYPED, YH>;
  using ST = CmAct<TYPED, SH>;
  const int qn = p.C >> 2;
  const int nbx = (p.WO + 3) >> 2, nby = (p.HO + 1) >> 1;
  const size_t total = (size_t)p.B * nby * nbx * qn;
  const float f0 = p.fs, f1 = 3.0f * p.fs;
  const float ns = (EPI == 1 && p.noise) ? p.noise_strength[0] : 0.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c4 = (int)(i % qn);
    size_t blk = i / qn;
    int smp = 0;
    if constexpr (SAMP) { smp = (int)(blk % S); blk /= S; }
    const int bx = (int)(blk % nbx); blk /= nbx;
    const int by = (int)(blk % nby);
    const int bi = (int)(blk / nby);                             // batch index of the skip tensor (SAMP: the image)
    const int b = SAMP ? bi * S + smp : bi;                      // batch index of x, y and the noise
    const int x0 = bx * 4, y0 = by * 2;
    const auto xb = XT::at(p.x, (size_t)b * p.H * p.W * p.C, c4);
    // EPI 1: the skip tensor and the noise plane of the 2 x 4 output block are requested first, so that they travel with
    // the 35 window loads instead of after the arithmetic that needs them last; the skip block stays in its stored form until it
    // is added
    typename ST::raw4 sk[2][4];
    float nz[2][4];
    f4 bias4 = {0.f, 0.f, 0.f, 0.f};                             // (read here, not between the stores below: a load behind a store waits for that store)
    if constexpr (EPI == 1) {
      bias4 = ld4(p.bias + c4 * 4);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int oy = y0 + r, ox = x0 + c;
          const bool ok = oy < p.HO && ox < p.WO;
          sk[r][c] = ST::zero();
          nz[r][c] = 0.0f;
          if (ok && p.skip) {
            const auto sp = ST::at(p.skip, (((size_t)bi * p.HO + oy) * p.WO + ox) * p.C, c4);
            sk[r][c] = SAMP ? ST::ld(sp) : ST::ld_once(sp);      // (S samples share an image's skip pixels: a plain load, not the read-once form)
          }
          if (ok && p.noise) nz[r][c] = p.noise[(size_t)b * p.noise_bstride + (size_t)oy * p.WO + ox];
        }
    }
    f4 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int iy = y0 - p.pad + r;
      const bool yok = iy >= 0 && iy < p.H;
      typename XT::raw4 raw[7];
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        const int ix = x0 - p.pad + c;
        raw[c] = XT::zero();
        if (yok && ix >= 0 && ix < p.W) raw[c] = XT::ld(XT::at(xb, ((size_t)iy * p.W + ix) * p.C));
      }
      f4 v[7];
#pragma unroll
      for (int c = 0; c < 7; ++c) v[c] = XT::cvt(raw[c]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f4 h = (v[c] + v[c + 3]) * f0 + (v[c + 1] + v[c + 2]) * f1;
        if (r < 4) acc[0][c] = acc[0][c] + h * ((r == 0 || r == 3) ? f0 : f1);
        if (r > 0) acc[1][c] = acc[1][c] + h * ((r == 1 || r == 4) ? f0 : f1);
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int oy = y0 + r;
      if (oy >= p.HO) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ox = x0 + c;
        if (ox >= p.WO) continue;
        const size_t o = (((size_t)b * p.HO + oy) * p.WO + ox) * p.C + c4 * 4;
        f4 v = acc[r][c];
        if constexpr (EPI == 1) {
          if (p.noise) v = v + MIGAN_FMUL_RN(nz[r][c], ns);
          v = act4(v + bias4);
          if (p.skip) v = v + ST::cvt(sk[r][c]);
        }
        YT::st(YT::at(p.y, o), v);
      }
    }
  }
