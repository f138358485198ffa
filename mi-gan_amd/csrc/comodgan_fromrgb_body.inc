// Body of cm_fromrgb_kernel and cm_fromrgb_h_kernel (comodgan_kernels.hpp), included into each like comodgan_fir_body.inc.
// The enclosing kernel supplies p (its CmFromRgbArgs) and YH: the output p.y holds _Float16.
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
  for (size_t pix = (size_t)blockIdx.x * ppb + threadIdx.x / qn; pix < npix; pix += (size_t)gridDim.x * ppb) {
    const size_t bi = pix / plane, rem = pix % plane;
    const float* xp = p.x + bi * 4 * plane + rem;
    const float x0 = xp[0], x1 = xp[plane], x2 = xp[2 * plane], x3 = xp[3 * plane];
    f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (x0 * w[j].x + x1 * w[j].y + x2 * w[j].z + x3 * w[j].w) + bias[j];
    if constexpr (YH) Io<2>::st(reinterpret_cast<char*>(reinterpret_cast<unsigned short*>(p.y) + pix * p.C + c4 * 4), 0u, act4(v));
    else st4(p.y + pix * p.C + c4 * 4, act4(v));
  }
