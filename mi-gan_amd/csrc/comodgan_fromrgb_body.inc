// Body of cm_fromrgb_kernel, cm_fromrgb_h_kernel and their _u8 twins (comodgan_kernels.hpp), included into each like
// comodgan_fir_body.inc.  The enclosing kernel supplies p (its CmFromRgbArgs), YH: the output p.y holds _Float16, and U8 with
// u8_img / u8_mask: the network input is formed in registers from the caller's photo and mask bytes (pack_pixel) and p.x is unused.
  // a thread keeps one channel quad (its 4 x 4 weights and bias stay in registers) and walks pixels; 256 / (C/4) pixels per
  // workgroup step, consecutive lanes = consecutive channel quads of a pixel (1 KiB contiguous store per wave)
  const int qn = p.C >> 2;                      // 16 ... 256, divides 256
  const int c4 = (int)threadIdx.x % qn;
  const int ppb = 256 / qn;
  const size_t plane = (size_t)p.R * p.R;
  const size_t npix = (size_t)p.B * plane;
  f4 w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = ld4(p.w + (c4 * 4 + j) * 4) * p.wgain;
  const f4 bias = ld4(p.b + c4 * 4);
  // U8: the bytes of a pixel are requested one step ahead, before the store of the step in front of it: a load issued after a store
  // waits for it (vmcnt retires in order).  A photo is [B][R][R][3] and a mask [B][R][R]: pixel `pix` of the walk, no plane split
  u4v u8_next = u4v{0u, 0u, 0u, 0u};
  if constexpr (U8) {
    const size_t first = (size_t)blockIdx.x * ppb + threadIdx.x / qn;
    if (first < npix) u8_next = fetch_pixel_bytes(u8_img, u8_mask, first);
  }
  for (size_t pix = (size_t)blockIdx.x * ppb + threadIdx.x / qn; pix < npix; pix += (size_t)gridDim.x * ppb) {
    float x0, x1, x2, x3;
    if constexpr (U8) {
      const u4v cur = u8_next;
      const size_t nxt = pix + (size_t)gridDim.x * ppb;
      if (nxt < npix) u8_next = fetch_pixel_bytes(u8_img, u8_mask, nxt);
      const f4 xq = pack_pixel_bytes(cur);
      x0 = xq.x; x1 = xq.y; x2 = xq.z; x3 = xq.w;
    } else {
      const size_t bi = pix / plane, rem = pix % plane;
      const float* xp = p.x + bi * 4 * plane + rem;
      x0 = xp[0]; x1 = xp[plane]; x2 = xp[2 * plane]; x3 = xp[3 * plane];
    }
    f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (x0 * w[j].x + x1 * w[j].y + x2 * w[j].z + x3 * w[j].w) + bias[j];
    if constexpr (YH) Io<2>::st(reinterpret_cast<char*>(reinterpret_cast<unsigned short*>(p.y) + pix * p.C + c4 * 4), 0u, act4(v));
    else st4(p.y + pix * p.C + c4 * 4, act4(v));
  }
