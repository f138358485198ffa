// Step 3 and the S result bytes per channel of crop pixel (py, px) in a post kernel that writes S outputs per crop pixel
// (pipe_post_samples_kernel, pipe_post_patches_kernel: migan_pipeline.hpp): the 5x5 blur of the pooled mask as 25 fp64 products in
// ky, kx order, reflected at the crop border, what depends on the pixel alone (pipe_post_coord), then the samples.  One text for
// both kernels, so that the blend below contracts the same way in both and the bytes match.
// From the enclosing kernel: p (.gauss, .R, .S, .y), pool, it.out, k, cw, ch, ty0, tx0, py, px, img[3] = the image's bytes at the
// pixel, and the destination's geometry: `plane` = its channel stride (sample stride 3 * plane), `at` = the pixel's offset in a plane.
  double acc = 0.0;
  for (int ky = 0; ky < 5; ++ky) {
    const int yy = pipe_reflect(py + ky - 2, ch) - (ty0 - 2);
    for (int kx = 0; kx < 5; ++kx) {
      const int xx = pipe_reflect(px + kx - 2, cw) - (tx0 - 2);
      acc += (double)p.gauss[ky * 5 + kx] * (double)pool[yy * kPostPW + xx];
    }
  }
  const PipePostCoord c = pipe_post_coord(p.R, cw, ch, py, px, acc);
  const size_t oplane3 = (size_t)3 * p.R * p.R;
  const float* y = p.y + (size_t)k * p.S * oplane3;
  const size_t oplane = (size_t)p.R * p.R;
  for (int s = 0; s < p.S; ++s) {
    unsigned char* o = it.out + (size_t)s * 3 * plane + at;
    // The blend of pipe_post_byte, img * mk + o * (1 - mk), is contracted by the compiler into one rounded product and an FMA, and
    // which product stays exact follows from where the two are computed.  img * mk does not depend on the sample: lifted out of
    // this loop it would be the rounded one, the other way round than in pipe_post_pixel, and a result next to an integer would
    // differ from pipe_post_batch_kernel's by one.  With mk opaque in every pass both products are formed here, as there.
    PipePostCoord cs = c;
    MIGAN_OPAQUE_F(cs.mk);
#pragma unroll
    for (int ch3 = 0; ch3 < 3; ++ch3) {
      float t[4];
      pipe_post_taps(y + ((size_t)s * 3 + ch3) * oplane, p.R, cs, t);
      o[ch3 * plane] = pipe_post_byte(t, cs, img[ch3]);
    }
  }
