// Body of cm_torgb_kernel<LPP>, cm_torgb_h_kernel<LPP>, their _parts twins and their _u8 twins (comodgan_kernels.hpp), included into
// each like comodgan_fir_body.inc.  The enclosing kernel supplies p (its CmRgbArgs), LPP, XH: the feature map p.x holds _Float16,
// PARTS: torgb(x) before the running image is added goes to rgb_out as well, and U8 with u8_img / u8_mask / u8_out / u8_S: the
// image is not stored to p.img_out but composed over the caller's photo (compose_pixel) into HWC bytes, row b against photo b / u8_S.
  static_assert(LPP == 4 || LPP == 8 || LPP == 16, "lanes per pixel");
  const int sub = threadIdx.x & (LPP - 1);
  const size_t pixel = ((size_t)blockIdx.x * 256 + threadIdx.x) / LPP;
  const size_t plane = (size_t)p.H * p.W;
  const size_t npix = (size_t)p.B * plane;
  const bool ok = pixel < npix;
  float r0 = 0.f, r1 = 0.f, r2 = 0.f;
  const int b = ok ? (int)(pixel / plane) : 0;
  // U8: lane ch of the group requests byte ch of the photo's pixel and its mask byte ahead of the channel walk; nothing uses them
  // before the store
  unsigned u8_px = 0u, u8_mk = 0u;
  if constexpr (U8) {
    if (ok && sub < 3) {
      const size_t src = (size_t)(b / u8_S) * plane + pixel % plane;
      u8_px = u8_img[src * 3 + sub];
      u8_mk = u8_mask[src];
    }
  }
  if (ok) {
    // the pixel's channels, fp16 or fp32, each in the element arithmetic its symbol has always had: unified they are the same
    // addresses and other code (profiles/comodgan_stream_bodies.md)
    const char* xp = XH ? reinterpret_cast<const char*>(reinterpret_cast<const unsigned short*>(p.x) + pixel * p.C)
                        : reinterpret_cast<const char*>(p.x + pixel * p.C);
    const float* w = p.wm + (size_t)b * 3 * p.C;
    for (int q = sub; q < (p.C >> 2); q += LPP) {
      const f4 v = XH ? Io<2>::cvt(Io<2>::ld(xp, (unsigned)q * 8u)) : ld4(reinterpret_cast<const float*>(xp) + q * 4);
      const f4 w0 = ld4(w + q * 4), w1 = ld4(w + p.C + q * 4), w2 = ld4(w + 2 * p.C + q * 4);
      // scalar FMA chains, not SLP-vectorised packed-fp32 dot products (profiles/r02_torgb_packed_f32_hazard.md)
      float a0, a1, a2;
      torgb_partial(v, w0, w1, w2, a0, a1, a2);
      r0 += a0;
      r1 += a1;
      r2 += a2;
    }
  }
#pragma unroll
  for (int s = LPP / 2; s >= 1; s >>= 1) {
    r0 += __shfl_xor(r0, s);
    r1 += __shfl_xor(r1, s);
    r2 += __shfl_xor(r2, s);
  }
  if (ok && sub < 3) {
    const int rem = (int)(pixel % plane);
    const int oy = rem / p.W, ox = rem % p.W;
    const float sum = sub == 0 ? r0 : (sub == 1 ? r1 : r2);
    float up = 0.0f;
    if (p.img_prev) up = up_prev3(p.img_prev + ((size_t)b * 3 + sub) * (plane >> 2), p.H >> 1, p.W >> 1, oy, ox);
    if constexpr (U8) {
      // compose_pixel's arithmetic on one channel: a known pixel keeps the photo's byte
      u8_out[pixel * 3 + sub] = u8_mk == 255u ? (unsigned char)u8_px : unit_to_u8(up + (sum + p.bias[sub]));
    } else if (PARTS) {
      // both stores behind every load: a load issued after a store waits for it (vmcnt retires in order)
      const float rgb = sum + p.bias[sub];
      rgb_out[((size_t)b * 3 + sub) * plane + rem] = rgb;
      p.img_out[((size_t)b * 3 + sub) * plane + rem] = up + rgb;
    } else {
      p.img_out[((size_t)b * 3 + sub) * plane + rem] = up + (sum + p.bias[sub]);
    }
  }
