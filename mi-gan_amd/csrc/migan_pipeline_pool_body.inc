// Steps 1 and 2 of a post kernel that writes S outputs per crop pixel (pipe_post_samples_kernel, pipe_post_patches_kernel:
// migan_pipeline.hpp), for the tile whose origin is (ty0, tx0) in crop coordinates: the mask window, 0 outside the crop, then its
// 3x3 max.  Ends behind the barrier that publishes `pool`.  One text for both kernels, so that both hold the same instructions.
// From the enclosing kernel: win, pool (LDS), it (.mask, .W), x_min, y_min, cw, ch, ty0, tx0, t.
  for (int e = t; e < kPostWH * kPostWW; e += kThreads) {
    const int cy = ty0 - 3 + e / kPostWW, cx = tx0 - 3 + e % kPostWW;
    win[e] = (cy >= 0 && cy < ch && cx >= 0 && cx < cw) ? it.mask[(size_t)(y_min + cy) * it.W + x_min + cx] : (unsigned char)0;
  }
  __syncthreads();
  for (int e = t; e < kPostPH * kPostPW; e += kThreads) {
    const unsigned char* w0 = win + e / kPostPW * kPostWW + e % kPostPW;
    int m = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int v = w0[dy * kPostWW + dx];
        m = v > m ? v : m;
      }
    pool[e] = (unsigned char)m;
  }
  __syncthreads();
