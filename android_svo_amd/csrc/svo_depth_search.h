// svo_depth_search.h -- the wave-per-four-seeds pixel stage: warp::warpAffine of the reference patch into LDS and the ZMSSD search
// along the epipolar line, with the hand-over to the alignment stage.
#pragma once
#include "svo_depth_types.h"
namespace {
// 8x8 ZMSSD of the LDS reference patch against the image patch whose top-left is `p`
// (I/patch_score.h:186-219: integer exact).
SVO_DEV int zmssd_8x8(const uint8_t* __restrict__ p, int stride, const uint32_t* patch_words, int sumA, int sumAA) {
  uint32_t sumB = 0, sumBB = 0, sumAB = 0;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const uint8_t* row = p + y * stride;
    uint32_t w0, w1;
    __builtin_memcpy(&w0, row, 4);
    __builtin_memcpy(&w1, row + 4, 4);
    const uint32_t a0 = patch_words[2 * y], a1 = patch_words[2 * y + 1];
    sumB = __builtin_amdgcn_udot4(w0, 0x01010101u, sumB, false);
    sumB = __builtin_amdgcn_udot4(w1, 0x01010101u, sumB, false);
    sumBB = __builtin_amdgcn_udot4(w0, w0, sumBB, false);
    sumBB = __builtin_amdgcn_udot4(w1, w1, sumBB, false);
    sumAB = __builtin_amdgcn_udot4(w0, a0, sumAB, false);
    sumAB = __builtin_amdgcn_udot4(w1, a1, sumAB, false);
  }
  const int sB = (int)sumB, sBB = (int)sumBB, sAB = (int)sumAB;
  return sumAA - 2 * sAB + sBB - (sumA * sumA - 2 * sumA * sB + sB * sB) / 64;
}

// ---- image windows in LDS -------------------------------------------------------------------------------------
// Both pixel phases of the search kernel gather bytes around one place of an image: the 100 bilinear samples of the
// affine warp, and the up to 16 overlapping 8x8 candidate patches of one chunk of the epipolar walk.  Read straight
// from memory that is 14 + 16 scattered load instructions per lane with ~40 cache-line accesses each, and the kernel
// is bound by L1 address processing (PMC: 0.8 line accesses per cycle and CU, TA busy 69 %).  Instead the 16 lanes of
// a seed copy the bounding box of what they need -- at most WIN_ROWS rows of WIN_PITCH bytes, one or two unaligned
// 16-byte loads per row, one row (two if the box is taller than 16) per lane -- into LDS and gather from there.  A box
// that does not fit (a strongly scaled warp, a segment steeper than the chunk allows) falls back to the direct loads.
constexpr int WIN_PITCH = 32;
constexpr int WIN_ROWS = 32;
constexpr int WIN_BYTES = WIN_ROWS * WIN_PITCH;

// lane cl (0..15) of a seed copies rows cl and cl + 16 of the h x WIN_PITCH box whose top-left byte is `src`.
// (Round 4 tried two lanes per row -- neighbouring lanes reading the two 16-byte halves of one row, four passes of eight
// rows, so that the address unit sees half as many cache lines per load: the kernel ran 23 % (100 k seeds) and 43 % (1 M
// seeds) SLOWER, same-box A/B; four conditional single-load blocks instead of two double-load ones.  Kept as it was.)
SVO_DEV void win_fill(const uint8_t* __restrict__ src, int pitch, int h, int cl, uint8_t* win) {
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = cl + 16 * half;
    if (r < h) {
      const uint8_t* p = src + (size_t)r * pitch;
      uint4 a, b;
      __builtin_memcpy(&a, p, 16);                       // unaligned global_load_dwordx4
      __builtin_memcpy(&b, p + 16, 16);
      *reinterpret_cast<uint4*>(win + r * WIN_PITCH) = a;
      *reinterpret_cast<uint4*>(win + r * WIN_PITCH + 16) = b;
    }
  }
}

// min / max over the 16 lanes of a DPP row, every lane gets it (the reductions of row16_sum with another operator)
SVO_DEV int row16_min(int v) {
  v = min(v, dpp_quad<0xB1>(v)); v = min(v, dpp_quad<0x4E>(v)); v = min(v, dpp_quad<0x141>(v)); v = min(v, dpp_quad<0x140>(v));
  return v;
}
SVO_DEV int row16_max(int v) {
  v = max(v, dpp_quad<0xB1>(v)); v = max(v, dpp_quad<0x4E>(v)); v = max(v, dpp_quad<0x141>(v)); v = max(v, dpp_quad<0x140>(v));
  return v;
}

// zmssd_8x8 with the candidate's 8x8 patch taken from an LDS window: `row0` = window row of the patch's first row,
// ox = byte offset of its first column (any value 0 .. WIN_PITCH - 8; dword-aligned reads + v_alignbyte)
SVO_DEV int zmssd_8x8_win(const uint8_t* row0, int ox, const uint32_t* patch_words, int sumA, int sumAA) {
  uint32_t sumB = 0, sumBB = 0, sumAB = 0;
  const int sh = ox & 3;
  const uint32_t* base = reinterpret_cast<const uint32_t*>(row0 + (ox & ~3));
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const uint32_t* r = base + y * (WIN_PITCH / 4);
    const uint32_t d0 = r[0], d1 = r[1], d2 = r[2];       // d2 may belong to the next row (or the pad): unused when sh == 0
    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh), w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
    const uint32_t a0 = patch_words[2 * y], a1 = patch_words[2 * y + 1];
    sumB = __builtin_amdgcn_udot4(w0, 0x01010101u, sumB, false);
    sumB = __builtin_amdgcn_udot4(w1, 0x01010101u, sumB, false);
    sumBB = __builtin_amdgcn_udot4(w0, w0, sumBB, false);
    sumBB = __builtin_amdgcn_udot4(w1, w1, sumBB, false);
    sumAB = __builtin_amdgcn_udot4(w0, a0, sumAB, false);
    sumAB = __builtin_amdgcn_udot4(w1, a1, sumAB, false);
  }
  const int sB = (int)sumB, sBB = (int)sumBB, sAB = (int)sumAB;
  return sumAA - 2 * sAB + sBB - (sumA * sumA - 2 * sumA * sB + sB * sB) / 64;
}

// Four seeds per wave, 16 per 256-thread block.  Three phases per wave:
//   A  one seed at a time, all 64 lanes: warp::warpAffine of the 10x10 reference patch into LDS (lanes = pixels)
//   B  the four seeds at once, 16 lanes each: ZMSSD search along the epipolar line (lane = candidate step; the
//      usual segment has ~11 steps, so a whole wave per seed left 5/6 of the lanes idle)
//   C  the four seeds at once, 16 lanes each: align2D / align1D (lane = 4 pixels of the 8x8 patch)
// (the body: workgroup `block` of 256 threads, seeds [16 * block, 16 * block + 16); no block-level barrier inside -- every wave
// works on its own four seeds)
// (`cam_of_block`: the camera model of the block's records -- fr.cam, or the model of the block's camera where a pass has several)
SVO_DEV void df_search_block(const DfFrame& fr, const Cam& cam_of_block, const uint8_t* __restrict__ ref_base, size_t ref_pyr_bytes,
                             const uint8_t* __restrict__ cur_pyr, int n, const int32_t* __restrict__ level,
                             SeedRec* __restrict__ recs, uint32_t* __restrict__ pwb_t, int n_pad, int block) {
  __shared__ __attribute__((aligned(16))) uint8_t s_pwb[SEEDS_PER_BLOCK][112];
  __shared__ __attribute__((aligned(16))) uint32_t s_patch[SEEDS_PER_BLOCK][16];
  __shared__ double s_px[SEEDS_PER_BLOCK][2];
  __shared__ int s_do[SEEDS_PER_BLOCK], s_nz[SEEDS_PER_BLOCK];
  __shared__ __attribute__((aligned(16))) uint8_t s_win[SEEDS_PER_BLOCK * WIN_BYTES + 16];   // image windows (+ pad: see zmssd_8x8_win)
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform -> SGPRs
  const int lane = threadIdx.x & 63;
  const int i0 = (block * 4 + wib) * SEEDS_PER_WAVE;
  if (i0 >= n) return;                     // wave-uniform; no block-level barrier is used below
  const Cam cam = cam_of_block;
  // the wave's four records (384 contiguous bytes) and levels go to LDS in one round trip: every phase below reads
  // its per-seed parameters from there instead of paying a memory latency per dependent field access
  __shared__ __attribute__((aligned(16))) SeedRec s_rec[SEEDS_PER_BLOCK];
  __shared__ int s_level[SEEDS_PER_BLOCK];
  {
    const int n_here = n - i0 < SEEDS_PER_WAVE ? n - i0 : SEEDS_PER_WAVE;
    static_assert(sizeof(SeedRec) == 96, "six 16-byte words per record");
    const uint4* src = reinterpret_cast<const uint4*>(recs + i0);
    uint4* dst = reinterpret_cast<uint4*>(s_rec + wib * SEEDS_PER_WAVE);
    if (lane < 6 * n_here) dst[lane] = src[lane];
    if (lane >= 32 && lane < 32 + n_here) s_level[wib * SEEDS_PER_WAVE + lane - 32] = level[i0 + lane - 32];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  // ---------------- phase A: warp the reference patches ----------------
  bool any_search = false;
  for (int sidx = 0; sidx < SEEDS_PER_WAVE; ++sidx) {
    const int i = i0 + sidx;
    if (i >= n) break;                                   // wave-uniform
    const int slot = wib * SEEDS_PER_WAVE + sidx;
    const SeedRec* rp = s_rec + slot;
    const int path = rp->path;
    if (lane == 0) { s_do[slot] = (path == 0 || path == 3) ? 1 : 0; s_nz[slot] = 0; s_px[slot][0] = rp->uv0[0]; s_px[slot][1] = rp->uv0[1]; }
    any_search |= path == 1;
  }
  {
    // 16 lanes per seed, 7 samples per lane: the seed's warp parameters are read once per lane
    const int g = lane >> 4, cl = lane & 15;
    const int i = i0 + g;
    const bool have = i < n;
    const SeedRec* rp = s_rec + wib * SEEDS_PER_WAVE + (have ? g : 0);
    const int path = have ? rp->path : -1;
    if (path == 0 || path == 1 || path == 3) {
      const uint8_t* ref_pyr = ref_base + (size_t)rp->pad * ref_pyr_bytes;   // pad = reference keyframe slot
      const int level_ref = s_level[wib * SEEDS_PER_WAVE + g];
      const int search_level = rp->search_level;
      // warp::warpAffine of the 10x10 reference patch (matcher.cpp:83-116)
      const int rcols = cam.width >> level_ref, rrows = cam.height >> level_ref;
      const uint8_t* img_ref = ref_pyr + fr.ref_level_off[level_ref];
      const float a00 = rp->a00, a01 = rp->a01, a10 = rp->a10, a11 = rp->a11, prx = rp->prx, pry = rp->pry;
      const bool warp_nan = rp->warp_nan != 0;
      const float lscale = (float)(1 << search_level);
      uint8_t* pwb = s_pwb[wib * SEEDS_PER_WAVE + g];
      // The source footprint of the patch: the four corners bound every sample (each f32 operation of the affine map is
      // monotone in the patch coordinate), the samples that are interpolated lie in [0, rcols-1) x [0, rrows-1).
      uint8_t* win = s_win + (wib * SEEDS_PER_WAVE + g) * WIN_BYTES;
      int wx0 = 0, wy0 = 0;
      bool use_win = false;
      {
        float xmin = 0, xmax = 0, ymin = 0, ymax = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float ppx = (float)((c & 1) ? 4 : -5) * lscale, ppy = (float)((c & 2) ? 4 : -5) * lscale;
          const float qx = (a00 * ppx + a01 * ppy) + prx, qy = (a10 * ppx + a11 * ppy) + pry;
          xmin = c == 0 ? qx : fminf(xmin, qx); xmax = c == 0 ? qx : fmaxf(xmax, qx);
          ymin = c == 0 ? qy : fminf(ymin, qy); ymax = c == 0 ? qy : fmaxf(ymax, qy);
        }
        // (comparisons with a NaN are false: a NaN box, like a NaN warp, keeps the direct path, which zeroes the patch)
        if (!warp_nan && xmin > -1e6f && ymin > -1e6f && xmax < 1e6f && ymax < 1e6f) {
          wx0 = max((int)floorf(xmin), 0); wy0 = max((int)floorf(ymin), 0);
          const int wx1 = min((int)floorf(xmax), rcols - 2) + 1, wy1 = min((int)floorf(ymax), rrows - 2) + 1;
          const int ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;
          if (ww > 0 && wh > 0 && ww <= WIN_PITCH && wh <= WIN_ROWS) {
            use_win = true;
            win_fill(img_ref + (size_t)wy0 * rcols + wx0, rcols, wh, cl, win);
          }
        }
      }
      // Two passes so that the 7 x 2 loads of a lane are in flight together (one memory latency instead of seven):
      // first every sample's address and weights -- a sample that is not interpolated reads offset 0 of the level,
      // which is always valid memory -- then the arithmetic of vk::interpolateMat_8u (I/vision.h:19-36) in its order.
      float w00[7], w01[7], w10[7], w11[7];
      unsigned r0[7], r1[7];
      bool ok[7];
      int woff[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int k = cl + 16 * j;
        const int yy = k / 10, xx = k - yy * 10;
        float ppx = (float)(xx - 5), ppy = (float)(yy - 5);
        ppx *= lscale;
        ppy *= lscale;
        const float qx = (a00 * ppx + a01 * ppy) + prx;
        const float qy = (a10 * ppx + a11 * ppy) + pry;
        // the reference keeps the previous seed's patch when the inverse warp is NaN and reads out of bounds when
        // qx/qy are NaN (inf inverse of a singular A); such samples are 0 here
        ok[j] = k < 100 && !warp_nan && qx >= 0 && qy >= 0 && qx < rcols - 1 && qy < rrows - 1;
        const float u = ok[j] ? qx : 0.0f, v = ok[j] ? qy : 0.0f;
        const int x = (int)floorf(u), y = (int)floorf(v);
        const float subpix_x = u - x, subpix_y = v - y;
        w00[j] = (1.0f - subpix_x) * (1.0f - subpix_y);
        w01[j] = (1.0f - subpix_x) * subpix_y;
        w10[j] = subpix_x * (1.0f - subpix_y);
        w11[j] = 1.0f - w00[j] - w01[j] - w10[j];
        woff[j] = ok[j] ? (y - wy0) * WIN_PITCH + (x - wx0) : 0;
        if (!use_win) {
          const uint8_t* ptr = img_ref + y * rcols + x;
          typedef unsigned short __attribute__((aligned(1))) u16u;
          r0[j] = *reinterpret_cast<const u16u*>(ptr);            // the two neighbours of a row in one unaligned load
          r1[j] = *reinterpret_cast<const u16u*>(ptr + rcols);
        }
      }
      if (use_win) {
        // the window of this seed was written by its own 16 lanes: order the LDS writes before the gathers
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      }
      if (use_win) {
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const uint8_t* q = win + woff[j];
          r0[j] = (unsigned)q[0] | ((unsigned)q[1] << 8);
          r1[j] = (unsigned)q[WIN_PITCH] | ((unsigned)q[WIN_PITCH + 1] << 8);
        }
      }
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int k = cl + 16 * j;
        const float val = w00[j] * (float)(r0[j] & 0xff) + w01[j] * (float)(r1[j] & 0xff) + w10[j] * (float)(r0[j] >> 8) +
                          w11[j] * (float)(r1[j] >> 8);
        if (k < 100) pwb[k] = ok[j] ? (uint8_t)val : (uint8_t)0;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  // createPatchFromPatchWithBorder (matcher.cpp:138-147): lane = pixel of the 8x8 patch
#pragma unroll
  for (int sidx = 0; sidx < SEEDS_PER_WAVE; ++sidx) {
    const int slot = wib * SEEDS_PER_WAVE + sidx;
    reinterpret_cast<uint8_t*>(s_patch[slot])[lane] = s_pwb[slot][((lane >> 3) + 1) * 10 + (lane & 7) + 1];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  // ---------------- phase B: epipolar ZMSSD search, 16 lanes per seed ----------------
  if (any_search) {                                      // wave-uniform
    const int g = lane >> 4, cl = lane & 15, gbase = lane & 48;
    const int gi = i0 + g;
    const int slot = wib * SEEDS_PER_WAVE + g;
    const bool have = gi < n;
    const SeedRec* rp = s_rec + wib * SEEDS_PER_WAVE + (have ? g : 0);
    const bool live = have && rp->path == 1;
    const int search_level = rp->search_level;
    const int ccols = cam.width >> search_level;
    const double inv_level = 1.0 / (1 << search_level);
    const uint8_t* cur_img = cur_pyr + fr.cur_level_off[search_level];
    const uint32_t* patch_words = s_patch[slot];
    const double step[2] = {rp->step[0], rp->step[1]};
    const double uv0[2] = {rp->uv0[0], rp->uv0[1]};
    const int n_steps = live ? rp->n_steps + 1 : 0;      // ++n_steps (matcher.cpp:297)
    int n_max = n_steps;
    n_max = max(n_max, __shfl_xor(n_max, 16, 64));
    n_max = max(n_max, __shfl_xor(n_max, 32, 64));       // wave-uniform trip count
    // reference patch statistics (ZMSSD ctor, patch_score.h:49-61): 4 pixels per lane
    int sumA, sumAA;
    {
      const uint32_t w = patch_words[cl];
      sumA = row16_sum((int)__builtin_amdgcn_udot4(w, 0x01010101u, 0u, false));
      sumAA = row16_sum((int)__builtin_amdgcn_udot4(w, w, 0u, false));
    }
    unsigned long long best_key = ~0ull;
    int prev_tail_x = 0, prev_tail_y = 0;                // last_checked_pxi entering the chunk
    double uv_tail[2] = {uv0[0], uv0[1]};                // exact uv of step index chunk0 (slow path only)
    bool chain_exact = true;                             // uv_tail is current (no fast chunk has been taken yet)
    int n_zmssd = 0;
    for (int chunk0 = 0; chunk0 < n_max; chunk0 += 16) {
      const int idx = chunk0 + cl;
      const bool in_range = idx < n_steps;
      // The serial loop produces uv_i by repeated addition (matcher.cpp:299).  uv0 + i*step differs from it by
      // < 1e-13 relative, i.e. < 1e-10 px: if every candidate of the chunk is farther than 1e-7 px from a
      // rounding boundary of (int)(px/2^L + 0.5) the integer pixel is the same and the chain is not needed.
      double uv[2] = {uv0[0] + (double)idx * step[0], uv0[1] + (double)idx * step[1]};
      double pxs[2];
      world2cam_uv(cam, uv[0], uv[1], pxs);
      double tx = pxs[0] * inv_level + 0.5, ty = pxs[1] * inv_level + 0.5;       // division by 2^L, exact
      const bool risky = in_range && !(fabs(tx - rint(tx)) > 1e-7 && fabs(ty - rint(ty)) > 1e-7);
      const bool group_risky = ((__ballot(risky) >> gbase) & 0xffffull) != 0ull;      // uniform within the 16 lanes
      if (group_risky) {
        // exact replay of the chain for this chunk: bring the tail to chunk0, then lane l adds `step` l times
        if (!chain_exact) {
          uv_tail[0] = uv0[0]; uv_tail[1] = uv0[1];
          for (int k = 0; k < chunk0; ++k) { uv_tail[0] += step[0]; uv_tail[1] += step[1]; }
        }
        uv[0] = uv_tail[0]; uv[1] = uv_tail[1];
        for (int k = 0; k < 15; ++k) {
          if (k < cl) { uv[0] += step[0]; uv[1] += step[1]; }
        }
        uv_tail[0] = __shfl(uv[0], gbase + 15, 64) + step[0];
        uv_tail[1] = __shfl(uv[1], gbase + 15, 64) + step[1];
        chain_exact = true;
        world2cam_uv(cam, uv[0], uv[1], pxs);
        tx = pxs[0] * inv_level + 0.5; ty = pxs[1] * inv_level + 0.5;
      } else {
        chain_exact = false;
      }
      const int pxi_x = (int)tx, pxi_y = (int)ty;
      // dedupe against the previous step (matcher.cpp:306-308): it never changes the arg-min, only the
      // count of evaluations, which we keep for the work counters
      int prev_x = __shfl_up(pxi_x, 1, 64), prev_y = __shfl_up(pxi_y, 1, 64);
      if (cl == 0) { prev_x = prev_tail_x; prev_y = prev_tail_y; }
      const bool dup = (pxi_x == prev_x && pxi_y == prev_y);
      const bool inframe = is_in_frame_level(cam, pxi_x, pxi_y, 8, search_level);
      int score = 0x7fffffff;
      const bool eval = in_range && !dup && inframe;
      // bounding box of the chunk's candidate patches (uniform within the 16 lanes): if it fits, one window fill
      // replaces the 16 row loads of every candidate
      const int bx0 = row16_min(eval ? pxi_x : 0x7fffffff), bx1 = row16_max(eval ? pxi_x : -0x7fffffff);
      const int by0 = row16_min(eval ? pxi_y : 0x7fffffff), by1 = row16_max(eval ? pxi_y : -0x7fffffff);
      const bool any_eval = bx1 >= bx0;
      const bool fits = any_eval && bx1 - bx0 + 8 <= WIN_PITCH && by1 - by0 + 8 <= WIN_ROWS;
      uint8_t* win = s_win + slot * WIN_BYTES;
      if (chunk0 > 0) {                                    // wave-uniform: the window of the previous chunk has been read
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
      if (fits) win_fill(cur_img + (size_t)(by0 - 4) * ccols + (bx0 - 4), ccols, by1 - by0 + 8, cl, win);
      if (eval) {
        if (fits) {
          score = zmssd_8x8_win(win + (pxi_y - by0) * WIN_PITCH, pxi_x - bx0, patch_words, sumA, sumAA);
        } else {
          const uint8_t* cp = cur_img + (pxi_y - 4) * ccols + (pxi_x - 4);
          score = zmssd_8x8(cp, ccols, patch_words, sumA, sumAA);
        }
      }
      n_zmssd += __popcll((__ballot(eval) >> gbase) & 0xffffull);
      if (eval && score < ZMSSD_THRESHOLD) {
        const unsigned long long key = ((unsigned long long)(unsigned)score << 32) | (unsigned long long)(unsigned)idx;
        if (key < best_key) best_key = key;
      }
      prev_tail_x = __shfl(pxi_x, gbase + 15, 64); prev_tail_y = __shfl(pxi_y, gbase + 15, 64);
    }
    // arg-min over the 16 lanes on (score, index): the smallest score, earliest index on ties
    unsigned long long k = best_key;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(k, o, 64);
      k = other < k ? other : k;
    }
    if (live) {
      double px_best[2] = {uv0[0], uv0[1]};
      const bool found = k != ~0ull;
      if (found) {
        // uv_best: replay the serial chain up to the winning index (uniform within the 16 lanes)
        const int best_idx = (int)(k & 0xffffffffull);
        double bu = uv0[0], bv = uv0[1];
        for (int t = 0; t < best_idx; ++t) { bu += step[0]; bv += step[1]; }
        world2cam_uv(cam, bu, bv, px_best);
      }
      if (cl == 0) { s_do[slot] = found ? 1 : 0; s_nz[slot] = n_zmssd; s_px[slot][0] = px_best[0]; s_px[slot][1] = px_best[1]; }
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  // ---------------- hand-over to the alignment stage ----------------
  // the warped 10x10 patch goes to memory word-transposed (word w of seed i at pwb_t[w * n_pad + i]: the lane-per-seed
  // alignment kernel reads it with fully coalesced loads), the start pixel and the "align this seed" flag into the record
  {
    const int g = lane >> 4, cl = lane & 15;
    const int gi = i0 + g;
    const int slot = wib * SEEDS_PER_WAVE + g;
    const bool have = gi < n;
    const SeedRec* rp = s_rec + wib * SEEDS_PER_WAVE + (have ? g : 0);
    const int path = have ? rp->path : -1;
    const bool live = path == 0 || path == 1 || path == 3;
    const bool do_align = live && s_do[slot] != 0;
    if (do_align) {
      const uint32_t* words = reinterpret_cast<const uint32_t*>(s_pwb[slot]);
      pwb_t[(size_t)cl * n_pad + gi] = words[cl];
      if (cl < 9) pwb_t[(size_t)(cl + 16) * n_pad + gi] = words[cl + 16];
    }
    if (live && cl == 0) {
      SeedRec* rp_out = recs + gi;
      rp_out->matched = do_align ? 2 : 0;                // 2 = "to be aligned" (df_align_kernel settles it to 0 / 1)
      if (path != 3) { rp_out->step[0] = s_px[slot][0]; rp_out->step[1] = s_px[slot][1]; }   // path 3 keeps its direction there
      rp_out->n_zmssd = s_nz[slot]; rp_out->n_align = 0;
    }
  }
}

__global__ __launch_bounds__(256, 7) void df_search_kernel(
    DfFrame fr, const uint8_t* __restrict__ ref_base, size_t ref_pyr_bytes, const uint8_t* __restrict__ cur_pyr, int n,
    const int32_t* __restrict__ level, SeedRec* __restrict__ recs, uint32_t* __restrict__ pwb_t, int n_pad) {
  df_search_block(fr, fr.cam, ref_base, ref_pyr_bytes, cur_pyr, n, level, recs, pwb_t, n_pad, blockIdx.x);
}

// ---- the warp / search and alignment stages over the candidates of the cameras of a tracker (svo_track.hip; a lone tracker
// is a group of one): camera c's records are [c * cap, c * cap + n_c) of one record array (cap a multiple of the 16 items a block takes, so a block never
// straddles two cameras), n_c = counters[c * counter_stride] as the camera's planning kernel left it, its current image is
// slot c of the frame pyramid batch; the reference keyframe of an item is the slot in its record, as always.
__global__ __launch_bounds__(256, 7) void df_search_cams_kernel(
    DfFrame fr, const uint8_t* __restrict__ ref_base, size_t ref_pyr_bytes, const uint8_t* __restrict__ cur_base, size_t cur_pyr_bytes,
    int cap, const int* __restrict__ counters, int counter_stride, const int32_t* __restrict__ level, SeedRec* __restrict__ recs,
    uint32_t* __restrict__ pwb_t, int n_pad) {
  const int c = (int)(((long long)blockIdx.x * SEEDS_PER_BLOCK) / cap);
  int n_c = counters[(size_t)c * counter_stride];
  n_c = n_c < cap ? n_c : cap;
  df_search_block(fr, fr.cam, ref_base, ref_pyr_bytes, cur_base + (size_t)c * cur_pyr_bytes, c * cap + n_c, level, recs, pwb_t, n_pad, blockIdx.x);
}

// The same over the cameras a list names (a tracker group's subset call): slice j of the grid -- cap / 16 blocks -- takes camera
// c = cam_list[j], whose records, counters row and current image lie where c puts them; `eb` is the block's index in the
// all-cameras layout, which is what the records and the transposed patches are addressed by.
__global__ __launch_bounds__(256, 7) void df_search_listed_kernel(
    DfFrame fr, const uint8_t* __restrict__ ref_base, size_t ref_pyr_bytes, const uint8_t* __restrict__ cur_base, size_t cur_pyr_bytes,
    int cap, const int* __restrict__ counters, int counter_stride, const int32_t* __restrict__ level, SeedRec* __restrict__ recs,
    uint32_t* __restrict__ pwb_t, int n_pad, const int* __restrict__ cam_list) {
  const int per_cam = cap / SEEDS_PER_BLOCK;
  const int j = (int)blockIdx.x / per_cam;
  const int c = cam_list[j];
  const int eb = c * per_cam + ((int)blockIdx.x - j * per_cam);
  int n_c = counters[(size_t)c * counter_stride];
  n_c = n_c < cap ? n_c : cap;
  df_search_block(fr, fr.cam, ref_base, ref_pyr_bytes, cur_base + (size_t)c * cur_pyr_bytes, c * cap + n_c, level, recs, pwb_t, n_pad, eb);
}

// ---- the warp / search stage over the batches of several cameras (svo_hip_seed_batch_update_cameras_async): the 16 records of a
// block lie inside ONE job of the device-resident table (job boundaries are multiples of 256 records); the job names the slot
// of its camera's current image, the end of its records and its camera's model in the pass's camera table.
__global__ __launch_bounds__(256, 7) void df_search_jobs_kernel(
    DfFrame fr, const DfCamJob* __restrict__ jobs, const int* __restrict__ block_job, const DfCamModel* __restrict__ cams,
    const uint8_t* __restrict__ ref_base, size_t ref_pyr_bytes, const uint8_t* __restrict__ cur_base, size_t cur_pyr_bytes,
    const int32_t* __restrict__ level, SeedRec* __restrict__ recs, uint32_t* __restrict__ pwb_t, int n_pad) {
  const DfCamJob& C = jobs[block_job[blockIdx.x / (256 / SEEDS_PER_BLOCK)]];
  df_search_block(fr, cams[C.cam].cam, ref_base, ref_pyr_bytes, cur_base + (size_t)C.cur_slot * cur_pyr_bytes, C.job.first_block * 256 + C.job.n, level, recs, pwb_t,
                  n_pad, blockIdx.x);
}
}  // namespace
