// One crop per hole region (include/migan_pipeline_regions_hip.h), included by migan_pipeline.hpp inside namespace migan: the mask is
// split into regions on the device -- box maximum (dilation), connected-component labelling, a box per region -- and the pre / post
// steps run over a table of (image, box, label) rows, each row writing only the pixels of its own label.
//
//   find   regions_mask_resize_kernel   nearest resize of a mask of another size (pipe_mask_resize_pixel)
//          regions_dilate_rows_kernel   hole indicator, box maximum over 2 gap + 1 columns                         -> rowdil (1 byte / pixel)
//          regions_dilate_cols_kernel   box maximum over 2 gap + 1 rows -> D; parent[i] = i inside D, -1 outside
//          regions_label_tile_kernel    union-find inside a 32 x 32 tile in LDS; parent[i] = the tile-local root, as a global index
//          regions_merge_kernel         union of the pairs of neighbours that straddle a tile border, atomic minimum on `parent`
//          regions_roots_kernel         the pixels with parent[i] == i are appended to the item's root list (capped)
//          regions_sort_kernel          one thread sorts the <= 65 roots: region k = the k-th smallest root (raster order)
//          regions_labels_kernel        label map, and the extents of the hole pixels of every label (slot 0: of all of them)
//          regions_boxes_kernel         pipe_box per slot
//   rows   pipe_pre_rows_kernel, pipe_post_rows_kernel
//
// Union-find by label equivalence (Playne & Hawick 2018, Komura 2015): parent[i] <= i always, a root has parent[i] == i, and
// union(a, b) hangs the larger root under the smaller with an atomic minimum, following the value the atomic returns when another
// thread moved the root first.  A set's root is therefore its smallest linear index, whatever the order of the unions; a load that
// sees an older parent only walks a longer way.  32-bit integer atomics only.  Every phase that needs the previous one complete is a
// launch of its own, so no kernel waits for another workgroup.
#ifndef MIGAN_ATOMIC_MIN_I32
// the CPU emulator: the lanes of a workgroup share one OS thread, workgroups run on several
#define MIGAN_ATOMIC_MIN_I32(p, v) __atomic_fetch_min((p), (v), __ATOMIC_RELAXED)
#define MIGAN_ATOMIC_MAX_I32(p, v) __atomic_fetch_max((p), (v), __ATOMIC_RELAXED)
#define MIGAN_ATOMIC_ADD_I32(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define MIGAN_ATOMIC_OR_U32(p, v) __atomic_fetch_or((p), (v), __ATOMIC_RELAXED)
#define MIGAN_LOAD_AGENT_I32(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#endif

constexpr int kRegionsCap = 64;                       // max_regions <= kRegionsCap
constexpr int kRegionsGapMax = 64;                    // the halo of the two dilation kernels
constexpr int kRegionsFindMax = 16;                   // items per launch of the find kernels
constexpr int kRegTile = 32;                          // the labelling tile is kRegTile x kRegTile
// per item in scratch: the number of roots | the root list (max_regions + 1 entries used) | extents [max_regions + 1][4]
constexpr int kRegMetaList = 1, kRegMetaExt = 1 + (kRegionsCap + 1), kRegMetaInts = kRegMetaExt + 4 * (kRegionsCap + 1);

struct PipeRegionsItem {
  const unsigned char* mask_src;     // the caller's mask [mh][mw]
  unsigned char* mask_resized;       // its nearest resize to [H][W] in scratch, or null when (mh, mw) == (H, W)
  unsigned char* rowdil;             // [H][W] scratch: 1 where a hole pixel lies within `gap` columns in the same row
  int* parent;                       // [H][W] scratch: the union-find forest of D, -1 outside D
  unsigned char* labels;             // [H][W], the caller's label map
  int* meta;                         // [kRegMetaInts] scratch
  int H, W, mh, mw;
};
struct PipeRegionsArgs {
  PipeRegionsItem item[kRegionsFindMax];
  int first[kRegionsFindMax + 1];
  int* count;                        // [n]
  int* boxes;                        // [n][max_regions + 1][4]
  int n, R, padding, gap, max_regions;
};
static_assert(sizeof(PipeRegionsArgs) <= 2048, "the regions argument must stay well under the 4 KB kernel-argument limit");

MIGAN_DEVICE MIGAN_INLINE const unsigned char* regions_mask(const PipeRegionsItem& it) {
  return it.mask_resized ? it.mask_resized : it.mask_src;
}
// any bit of [a, b] set in the bit array `bits` (32 per word); 0 <= a <= b inside the array
MIGAN_DEVICE MIGAN_INLINE bool regions_bits_any(const unsigned* bits, int a, int b) {
  for (int w = a >> 5; w <= (b >> 5); ++w) {
    unsigned m = 0xffffffffu;
    if (w == (a >> 5)) m &= 0xffffffffu << (a & 31);
    if (w == (b >> 5)) m &= 0xffffffffu >> (31 - (b & 31));
    if (bits[w] & m) return true;
  }
  return false;
}
// union-find on `parent` (every entry touched is >= 0).  GLOBAL: the forest in global memory, shared by all workgroups -- loads that
// bypass the CU's cache see the other workgroups' atomics sooner; in LDS the workgroup's own
template <bool GLOBAL>
MIGAN_DEVICE MIGAN_INLINE int regions_load(const int* q) {
  if (GLOBAL) return MIGAN_LOAD_AGENT_I32(q);
  return *reinterpret_cast<const volatile int*>(q);
}
template <bool GLOBAL>
MIGAN_DEVICE MIGAN_INLINE int regions_root(const int* parent, int a) {
  int q = regions_load<GLOBAL>(parent + a);
  while (q != a) { a = q; q = regions_load<GLOBAL>(parent + a); }
  return a;
}
template <bool GLOBAL>
MIGAN_DEVICE MIGAN_INLINE void regions_union(int* parent, int a, int b) {
  for (;;) {
    a = regions_root<GLOBAL>(parent, a);
    b = regions_root<GLOBAL>(parent, b);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }                  // a > b: a goes under b
    const int old = MIGAN_ATOMIC_MIN_I32(parent + a, b);
    if (old == a) return;                                          // a was still a root: done
    a = old;                                                       // another thread moved a first: its new parent joins b's set
  }
}

// tiles of kThreads pixels of the items whose mask has another size than their image (the others have no tile)
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_mask_resize_kernel(const PipeRegionsArgs p) {
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeRegionsItem& it = p.item[k];
  pipe_mask_resize_pixel(it.mask_src, it.mh, it.mw, it.mask_resized, it.H, it.W, ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x);
}

// Row pass of the box maximum.  A workgroup owns kThreads pixels of one row; the hole indicator of those and of kRegionsGapMax
// columns either side goes into LDS as a bit array (the holes are few: one LDS atomic each), and a pixel tests the 2 gap + 1 bits
// around it in at most 5 words.  Columns outside the image hold no hole.  Tile 0 of an item also clears its root counter.
constexpr int kRegRowBits = kThreads + 2 * kRegionsGapMax, kRegRowWords = kRegRowBits / 32;
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_dilate_rows_kernel(const PipeRegionsArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned* bits = reinterpret_cast<unsigned*>(smem);                // [kRegRowWords]: bit e = column x0 - kRegionsGapMax + e
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeRegionsItem& it = p.item[k];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (it.W + kThreads - 1) / kThreads;
  const int y = tile / ntx, x0 = tile % ntx * kThreads;
  if (y >= it.H) return;                                             // (workgroup-uniform)
  const int t = (int)threadIdx.x;
  if (t < kRegRowWords) bits[t] = 0u;
  if (tile == 0 && t == 0) it.meta[0] = 0;
  __syncthreads();
  const unsigned char* row = regions_mask(it) + (size_t)y * it.W;
  for (int e = t; e < kRegRowBits; e += kThreads) {
    const int col = x0 - kRegionsGapMax + e;
    if (col >= 0 && col < it.W && row[col] != 255) MIGAN_ATOMIC_OR_U32(bits + (e >> 5), 1u << (e & 31));
  }
  __syncthreads();
  const int col = x0 + t;
  if (col < it.W)
    it.rowdil[(size_t)y * it.W + col] =
        regions_bits_any(bits, kRegionsGapMax + t - p.gap, kRegionsGapMax + t + p.gap) ? (unsigned char)1 : (unsigned char)0;
}

// Column pass.  A workgroup owns kRegTile columns x kRegColRows rows; per column, the rows of the tile and kRegionsGapMax either side
// as a bit array in LDS (an odd stride of words: the 32 columns of a half wave fall into different banks).  Writes the forest's
// initial state: a pixel of D is its own parent, any other pixel has none.
constexpr int kRegColRows = 64, kRegColBits = kRegColRows + 2 * kRegionsGapMax, kRegColStride = kRegColBits / 32 + 1;
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_dilate_cols_kernel(const PipeRegionsArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned* cols = reinterpret_cast<unsigned*>(smem);                // [kRegTile][kRegColStride]: bit r = row y0 - kRegionsGapMax + r
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeRegionsItem& it = p.item[k];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (it.W + kRegTile - 1) / kRegTile;
  const int y0 = tile / ntx * kRegColRows, x0 = tile % ntx * kRegTile;
  if (y0 >= it.H) return;                                            // (workgroup-uniform)
  const int t = (int)threadIdx.x;
  for (int e = t; e < kRegTile * kRegColStride; e += kThreads) cols[e] = 0u;
  __syncthreads();
  for (int e = t; e < kRegColBits * kRegTile; e += kThreads) {
    const int r = e / kRegTile, c = e % kRegTile;
    const int row = y0 - kRegionsGapMax + r, col = x0 + c;
    if (row >= 0 && row < it.H && col < it.W && it.rowdil[(size_t)row * it.W + col])
      MIGAN_ATOMIC_OR_U32(cols + c * kRegColStride + (r >> 5), 1u << (r & 31));
  }
  __syncthreads();
  const int c = t % kRegTile, col = x0 + c;
  for (int r = t / kRegTile; r < kRegColRows; r += kThreads / kRegTile) {
    const int row = y0 + r;
    if (row >= it.H || col >= it.W) continue;
    const int i = row * it.W + col;
    it.parent[i] = regions_bits_any(cols + c * kRegColStride, kRegionsGapMax + r - p.gap, kRegionsGapMax + r + p.gap) ? i : -1;
  }
}

// Union-find inside a kRegTile x kRegTile tile, in LDS (kRegTile^2 ints, 4 pixels per thread): every pixel of D joins its W, NW,
// N and NE neighbours in the tile.  The tile-local root is the set's smallest local index, which is also its smallest global index
// (both orders are row-major), so parent[i] = that pixel's global index keeps parent[i] <= i.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_label_tile_kernel(const PipeRegionsArgs p) {
  MIGAN_DYN_SMEM(smem);
  int* lab = reinterpret_cast<int*>(smem);                           // [kRegTile * kRegTile], -1 outside D
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeRegionsItem& it = p.item[k];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (it.W + kRegTile - 1) / kRegTile;
  const int y0 = tile / ntx * kRegTile, x0 = tile % ntx * kRegTile;
  if (y0 >= it.H) return;                                            // (workgroup-uniform)
  const int t = (int)threadIdx.x;
  for (int l = t; l < kRegTile * kRegTile; l += kThreads) {
    const int row = y0 + l / kRegTile, col = x0 + l % kRegTile;
    lab[l] = (row < it.H && col < it.W && it.parent[row * it.W + col] >= 0) ? l : -1;
  }
  __syncthreads();
  for (int l = t; l < kRegTile * kRegTile; l += kThreads) {
    if (lab[l] < 0) continue;
    const int ly = l / kRegTile, lx = l % kRegTile;
    if (lx > 0 && lab[l - 1] >= 0) regions_union<false>(lab, l, l - 1);
    if (ly > 0) {
      if (lab[l - kRegTile] >= 0) regions_union<false>(lab, l, l - kRegTile);
      if (lx > 0 && lab[l - kRegTile - 1] >= 0) regions_union<false>(lab, l, l - kRegTile - 1);
      if (lx < kRegTile - 1 && lab[l - kRegTile + 1] >= 0) regions_union<false>(lab, l, l - kRegTile + 1);
    }
  }
  __syncthreads();
  for (int l = t; l < kRegTile * kRegTile; l += kThreads) {
    if (lab[l] < 0) continue;
    const int r = regions_root<false>(lab, l);
    it.parent[(y0 + l / kRegTile) * it.W + x0 + l % kRegTile] = (y0 + r / kRegTile) * it.W + x0 + r % kRegTile;
  }
}

// Union across tile borders, on the global forest.  A pair (pixel, its W / NW / N / NE neighbour) straddles a border only when the
// pixel lies in the top row, the left column or (NE) the right column of its tile: 3 kRegTile threads per tile look at those.  The
// union is exact (a set keeps one root however many tiles it crosses and in whatever order the pairs arrive): one pass is enough.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_merge_kernel(const PipeRegionsArgs p) {
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeRegionsItem& it = p.item[k];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (it.W + kRegTile - 1) / kRegTile;
  const int y0 = tile / ntx * kRegTile, x0 = tile % ntx * kRegTile;
  const int t = (int)threadIdx.x;
  if (y0 >= it.H || t >= 3 * kRegTile) return;
  const int ly = t < kRegTile ? 0 : t % kRegTile, lx = t < kRegTile ? t : (t < 2 * kRegTile ? 0 : kRegTile - 1);
  const int row = y0 + ly, col = x0 + lx;
  if (row >= it.H || col >= it.W) return;
  const int i = row * it.W + col;
  if (it.parent[i] < 0) return;
  const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, -1, 0, 1};
  for (int d = 0; d < 4; ++d) {
    const int qy = row + dy[d], qx = col + dx[d];
    if (qy < 0 || qx < 0 || qx >= it.W) continue;
    if (qy / kRegTile == row / kRegTile && qx / kRegTile == col / kRegTile) continue;      // same tile: regions_label_tile_kernel's
    const int q = qy * it.W + qx;
    if (it.parent[q] >= 0) regions_union<true>(it.parent, i, q);          // (parent[q] >= 0 never changes sign)
  }
}

// tiles of kThreads pixels: a root appends itself; the list holds max_regions + 1 entries, the counter goes on counting
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_roots_kernel(const PipeRegionsArgs p) {
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeRegionsItem& it = p.item[k];
  const int i = ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x;
  if (i >= it.H * it.W || it.parent[i] != i) return;
  const int slot = MIGAN_ATOMIC_ADD_I32(it.meta, 1);
  if (slot <= p.max_regions) it.meta[kRegMetaList + slot] = i;
}

// one workgroup per item: thread 0 sorts the roots (the append order is arbitrary, the sorted order is the raster order of the
// regions' first pixels) and leaves the item's count, K or max_regions + 1, in meta[0] and in count[]; the others reset the extents
// to the reference's "nothing masked" values (:149-152)
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_sort_kernel(const PipeRegionsArgs p) {
  const PipeRegionsItem& it = p.item[blockIdx.x];
  const int t = (int)threadIdx.x;
  for (int e = t; e < 4 * (p.max_regions + 1); e += kThreads) it.meta[kRegMetaExt + e] = (e & 3) == 0 ? it.W : ((e & 3) == 2 ? it.H : 0);
  if (t != 0) return;
  int n = it.meta[0];
  if (n > p.max_regions) {
    n = p.max_regions + 1;
  } else {
    int* list = it.meta + kRegMetaList;
    for (int a = 1; a < n; ++a) {
      const int v = list[a];
      int b = a - 1;
      for (; b >= 0 && list[b] > v; --b) list[b + 1] = list[b];
      list[b + 1] = v;
    }
  }
  it.meta[0] = n;
  p.count[blockIdx.x] = n;
}

// Tiles of kThreads pixels: the label of a pixel of D is 1 + the rank of its root in the sorted list (0 for every pixel of an item
// with more regions than max_regions).  The extents of the hole pixels per label, and of all hole pixels in slot 0, are reduced in
// LDS with integer atomics -- a tile can hold several labels, so it is a table of slots, not one tree -- and the slots the tile
// touched go to the item's table with one global atomic each.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_labels_kernel(const PipeRegionsArgs p) {
  MIGAN_DYN_SMEM(smem);
  int* list = reinterpret_cast<int*>(smem);                          // [kRegionsCap + 1] sorted roots
  int* ext = list + kRegionsCap + 1;                                 // [kRegionsCap + 1][4] = {x_min, x_max, y_min, y_max}
  const int k = pipe_table_item(p, (int)blockIdx.x);
  const PipeRegionsItem& it = p.item[k];
  const int t = (int)threadIdx.x;
  const int count = it.meta[0], nslots = 4 * (p.max_regions + 1);
  const bool split = count <= p.max_regions;
  if (split && t < count) list[t] = it.meta[kRegMetaList + t];
  for (int e = t; e < nslots; e += kThreads) ext[e] = (e & 3) == 0 ? it.W : ((e & 3) == 2 ? it.H : 0);
  __syncthreads();
  const int i = ((int)blockIdx.x - p.first[k]) * kThreads + t;
  if (i < it.H * it.W) {
    int label = 0;
    if (split && it.parent[i] >= 0) {
      const int r = regions_root<true>(it.parent, i);
      int lo = 0, hi = count - 1;                                    // r is in the list: every root was appended
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < r) lo = mid + 1; else hi = mid;
      }
      label = lo + 1;
    }
    it.labels[i] = (unsigned char)label;
    if (regions_mask(it)[i] != 255) {
      const int x = i % it.W, y = i / it.W;
      for (int s = 0; s <= label; s += (label > 0 ? label : 1)) {    // slot 0, then the label's own
        MIGAN_ATOMIC_MIN_I32(ext + 4 * s, x); MIGAN_ATOMIC_MAX_I32(ext + 4 * s + 1, x);
        MIGAN_ATOMIC_MIN_I32(ext + 4 * s + 2, y); MIGAN_ATOMIC_MAX_I32(ext + 4 * s + 3, y);
      }
    }
  }
  __syncthreads();
  for (int e = t; e < nslots; e += kThreads) {
    const int v = ext[e];
    if ((e & 1) == 0) { if (v < ((e & 3) == 0 ? it.W : it.H)) MIGAN_ATOMIC_MIN_I32(it.meta + kRegMetaExt + e, v); }
    else if (v > 0) MIGAN_ATOMIC_MAX_I32(it.meta + kRegMetaExt + e, v);
  }
}

// one workgroup per item, thread s = slot s: pipe_box of the slot's extents; slot 0 is the reference's single box
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) regions_boxes_kernel(const PipeRegionsArgs p) {
  const PipeRegionsItem& it = p.item[blockIdx.x];
  const int s = (int)threadIdx.x;
  if (s > p.max_regions) return;
  const int count = it.meta[0];
  int box[4] = {0, 0, 0, 0};
  if (s == 0 || (count <= p.max_regions && s <= count)) {
    const int* e = it.meta + kRegMetaExt + 4 * s;
    pipe_box(e[0], e[1], e[2], e[3], it.W, it.H, p.R, p.padding, box);
  }
  int* out = p.boxes + ((size_t)blockIdx.x * (p.max_regions + 1) + s) * 4;
  out[0] = box[0]; out[1] = box[1]; out[2] = box[2]; out[3] = box[3];
}

// ---- pre / post over a table of rows ------------------------------------------------------------------------------------------------
// A row is (image, box, label), by value in the kernel argument like PipeBatchItem; the box is host data here (the caller read the
// boxes back to size the generator batch), so the post grid has exactly the crop's tiles.
constexpr int kPipeRowsMax = 32;
struct PipeRowItem {
  unsigned char* image;              // [3][H][W] uint8; post: read and written where labels == label
  const unsigned char* mask;         // [H][W], the full mask at the image's size
  const unsigned char* labels;       // [H][W]; not read when label == 0
  int H, W, label;
  int box[4];
};
struct PipeRowsArgs {
  PipeRowItem item[kPipeRowsMax];
  int first[kPipeRowsMax + 1];
  float* x;                          // pre: network input [n][4][R][R]
  const float* y;                    // post: network output [n][3][R][R]
  int n, R;
  float gauss[25];
};
static_assert(sizeof(PipeRowsArgs) <= 2304, "the rows argument must stay well under the 4 KB kernel-argument limit");

// cdiv(R * R, kThreads) tiles per row: pipe_pre_batch_kernel with the box in the argument
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_pre_rows_kernel(const PipeRowsArgs p) {
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out: the call changes this kernel's code)
  const PipeRowItem& it = p.item[k];
  if (!pipe_box_valid(it.box, it.H, it.W)) return;
  pipe_pre_pixel(it.image, it.mask, p.x + (size_t)k * 4 * p.R * p.R, it.H, it.W, p.R, it.box[0], it.box[1], it.box[2], it.box[3],
                 ((int)blockIdx.x - p.first[k]) * kThreads + (int)threadIdx.x);
}

// pipe_post_batch_kernel's tile scheme and arithmetic (the two LDS steps are migan_pipeline_pool_body.inc's text, the blur and
// pipe_post_pixel follow in its order) with the label test in front of the image read and the store.  A tile without a pixel of
// its label leaves before the window is loaded (workgroup-uniform: one LDS flag); a single-box row (label 0) has no test.
MIGAN_GLOBAL void MIGAN_LAUNCH_BOUNDS(256, 2) pipe_post_rows_kernel(const PipeRowsArgs p) {
  MIGAN_DYN_SMEM(smem);
  unsigned char* win = reinterpret_cast<unsigned char*>(smem);       // [kPostWH][kPostWW]: crop rows ty0 - 3 ..., columns tx0 - 3 ...
  unsigned char* pool = win + kPostWinBytes;                         // [kPostPH][kPostPW]: crop rows ty0 - 2 ..., columns tx0 - 2 ...
  int* any = reinterpret_cast<int*>(win + kPostLdsBytes);            // the tile holds a pixel of the row's label
  int k = 0;
  while (k + 1 < p.n && (int)blockIdx.x >= p.first[k + 1]) ++k;      // (wave-uniform; pipe_table_item, spelled out: the call changes this kernel's code)
  const PipeRowItem& it = p.item[k];
  if (!pipe_box_valid(it.box, it.H, it.W)) return;
  const int x_min = it.box[0], y_min = it.box[2], cw = it.box[1] - it.box[0], ch = it.box[3] - it.box[2];
  const int tile = (int)blockIdx.x - p.first[k], ntx = (cw + kPostTW - 1) / kPostTW;
  const int ty0 = tile / ntx * kPostTH, tx0 = tile % ntx * kPostTW;
  if (ty0 >= ch) return;                                             // (workgroup-uniform, like the returns above)
  const int t = (int)threadIdx.x;
  const int py = ty0 + t / kPostTW, px = tx0 + t % kPostTW;
  bool mine = py < ch && px < cw;
  if (it.label != 0) {                                               // (workgroup-uniform)
    if (t == 0) *any = 0;
    __syncthreads();
    mine = mine && it.labels[(size_t)(y_min + py) * it.W + x_min + px] == it.label;
    if (mine) *any = 1;                                              // (every writer stores the same value)
    __syncthreads();
    if (*any == 0) return;
  }
#include "migan_pipeline_pool_body.inc"                              // steps 1 and 2
  if (!mine) return;
  double acc = 0.0;
  for (int ky = 0; ky < 5; ++ky) {
    const int yy = pipe_reflect(py + ky - 2, ch) - (ty0 - 2);
    for (int kx = 0; kx < 5; ++kx) {
      const int xx = pipe_reflect(px + kx - 2, cw) - (tx0 - 2);
      acc += (double)p.gauss[ky * 5 + kx] * (double)pool[yy * kPostPW + xx];
    }
  }
  pipe_post_pixel(it.image, p.y + (size_t)k * 3 * p.R * p.R, it.H, it.W, p.R, x_min, y_min, cw, ch, py, px, acc);
}
