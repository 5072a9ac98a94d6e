/*
 * svo_hip.h -- C-ABI of libsvo_hip.so: the MI355X (gfx950) implementation of SVO's
 * data-parallel hot path (sparse image alignment, align2D, depth-filter update).
 *
 * This is the drop-in boundary: plain C types, pointers and sizes only.
 * The reference has no FFI layer -- its "operator API" is the public C++ surface of
 * svo::SparseImgAlign / svo::feature_alignment / svo::DepthFilter; the host-side C++
 * classes that keep those signatures and forward here live in include/svo_dropin/ and are
 * described in INTEGRATION.md.  Each entry point cites the reference interface it replaces
 * (paths relative to /root/reference/app/src/main/cpp/svo/, "I/" = include/svo/).
 *
 * Conventions
 *   - every function returns an int status (SVO_HIP_OK == 0, negative on error); nothing
 *     throws across the boundary, device errors never abort the calling thread;
 *   - SE3 poses are double[7] = {tx,ty,tz,qx,qy,qz,qw} (I/SE3.h, I/SO3.h member order);
 *   - images are 8-bit, row-major, stride == cols; level l of a pyramid is (w>>l) x (h>>l);
 *   - a context owns one HIP stream; every call on a context is enqueued on that stream and
 *     is asynchronous unless stated otherwise.  Contexts share no mutable state, so the
 *     tracking thread and the depth-filter thread of the reference (SURVEY 8b "Threading")
 *     each use their own context concurrently;
 *   - pointers named *_dev are DEVICE pointers (from svo_hip_malloc or any HIP allocator,
 *     e.g. a torch tensor's data_ptr); all others are host pointers that are copied in
 *     before the call returns and never retained.
 */
#ifndef SVO_HIP_H_
#define SVO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_HIP_OK 0
#define SVO_HIP_ERR_INVALID (-1)    /* bad argument (null, out of range, shape mismatch) */
#define SVO_HIP_ERR_DEVICE (-2)     /* a HIP runtime call failed: see svo_hip_last_error */
#define SVO_HIP_ERR_NOMEM (-3)
#define SVO_HIP_ERR_STATE (-4)      /* call sequence violated */

#define SVO_HIP_MAX_LEVELS 8
#define SVO_HIP_REDUCE_DOUBLES 32   /* per frame: 21 H (upper, row-major) + 6 Jres + chi2 sum + n_meas + pad */

typedef struct svo_hip_ctx svo_hip_ctx;
typedef struct svo_hip_pyramid svo_hip_pyramid;
typedef struct svo_hip_sia svo_hip_sia;

/* vk::PinholeCamera forward model (pinhole_camera.cpp:73-106): distortion != 0 enables the
 * 5-coefficient radtan model d = {k1,k2,p1,p2,k3} in world2cam.  cam2world (needed by the
 * epipolar matcher) is implemented for distortion == 0 only. */
typedef struct {
  int width, height;
  double fx, fy, cx, cy;
  double d[5];
  int distortion;
} svo_hip_camera;

/* ---- context / memory ------------------------------------------------------------------ */
/* stream: an existing hipStream_t to enqueue on (e.g. torch's current stream), or NULL to
 * create a private non-blocking stream. */
int svo_hip_ctx_create(svo_hip_ctx** out, int device, void* stream);
int svo_hip_ctx_destroy(svo_hip_ctx* ctx);
int svo_hip_ctx_sync(svo_hip_ctx* ctx);            /* hipStreamSynchronize on the context stream */
/* Memory bookkeeping of a context.  The library takes device / page-locked memory for a context's grow-only work areas
 * and for the blocks of its seed-batch pool (svo_hip_seed_batch_create / _destroy recycle blocks: the reference creates and
 * drops a keyframe's seeds at keyframe rate on the depth-filter thread, S/depth_filter.cpp:129-151,256-261, and hipFree
 * would synchronise the whole device under the tracking thread).  `allocator_calls` counts hipMalloc + hipHostMalloc calls,
 * `free_calls` hipFree + hipHostFree: both stay flat once the context has seen its working set (asserted over 20 keyframes
 * in tests/test_gpu_seed_batch.py).  svo_hip_ctx_trim returns the pool's free blocks to the driver (synchronises). */
typedef struct svo_hip_ctx_stats {
  unsigned long long allocator_calls, free_calls;
  unsigned long long seed_pool_free_device_bytes, seed_pool_free_host_bytes, scratch_bytes, staging_bytes;
  int seed_blocks_in_use, seed_blocks_free;
} svo_hip_ctx_stats;
int svo_hip_ctx_info(svo_hip_ctx* ctx, svo_hip_ctx_stats* out);
int svo_hip_ctx_trim(svo_hip_ctx* ctx);
void* svo_hip_ctx_stream(svo_hip_ctx* ctx);
const char* svo_hip_last_error(svo_hip_ctx* ctx);  /* text of the last failure on this context */
const char* svo_hip_version(void);
int svo_hip_device_count(int* count);

int svo_hip_malloc(svo_hip_ctx* ctx, void** dev_ptr, size_t bytes);
int svo_hip_free(svo_hip_ctx* ctx, void* dev_ptr);
/* page-locked host memory for image / feature staging: uploads from it are asynchronous DMA at link rate, uploads
 * from pageable memory are staged by the runtime (measured: profiles/r01_hbm_probe.json) */
int svo_hip_malloc_host(svo_hip_ctx* ctx, void** host_ptr, size_t bytes);
int svo_hip_free_host(svo_hip_ctx* ctx, void* host_ptr);
int svo_hip_memcpy_h2d(svo_hip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);   /* async */
int svo_hip_memcpy_d2h(svo_hip_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);   /* synchronises */
int svo_hip_copy_d2d(svo_hip_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);        /* async */
int svo_hip_memset(svo_hip_ctx* ctx, void* dst_dev, int value, size_t bytes);

/* The camera model exactly as every kernel evaluates it, over n host items (vk::PinholeCamera::world2cam for
 * camera-frame points xyz[n][3] and for unit-plane points uv[n][2], pinhole_camera.cpp:73-106; ::cam2world for
 * pixels px[n][2], :44-71; vk::AbstractCamera::isInFrame(obs[n][2], boundary) when level < 0, else
 * isInFrame(obs, boundary, level), I/abstract_camera.h:58-72).  Each input/output pair may be NULL.  Synchronises. */
int svo_hip_camera_batch(svo_hip_ctx* ctx, const svo_hip_camera* cam, int n, const double* xyz, const double* uv,
                         const double* px, const int32_t* obs, int boundary, int level, double* px_of_xyz,
                         double* px_of_uv, double* f_of_px, uint8_t* in_frame);

/* ---- image pyramids resident in HBM (Frame::img_pyr_, frame.cpp:63,186-195) ------------ */
/* A batch of `batch` pyramids of identical geometry, one contiguous allocation:
 * slot s, level l starts at s*pyr_bytes + level_offset[l]. */
int svo_hip_pyramid_create(svo_hip_ctx* ctx, int width, int height, int n_levels, int batch,
                           svo_hip_pyramid** out);
int svo_hip_pyramid_destroy(svo_hip_pyramid* pyr);
/* copy all levels from host (levels[l] has (w>>l)*(h>>l) bytes) */
int svo_hip_pyramid_upload(svo_hip_pyramid* pyr, int slot, const uint8_t* const* levels);
/* copy level 0 only and build levels 1.. on the device with the truncating 2x2 mean
 * (vk::halfSample scalar/NEON form, vision.cpp:49-67,89-110; frame_utils::createImgPyramid,
 * frame.cpp:186-195).  The x86 SSE2 form of the reference rounds differently (vision.cpp:33-37). */
int svo_hip_pyramid_upload_level0_and_build(svo_hip_pyramid* pyr, int slot, const uint8_t* level0);
int svo_hip_pyramid_download_level(svo_hip_pyramid* pyr, int slot, int level, uint8_t* out_host);
/* n_slots pyramids in the device layout (each pyr_bytes long, level l at svo_hip_pyramid_level_offset) in ONE
 * transfer: from page-locked memory this runs at link rate, where per-level uploads are latency-bound */
int svo_hip_pyramid_level_offset(const svo_hip_pyramid* pyr, int level, size_t* offset);
int svo_hip_pyramid_upload_packed(svo_hip_pyramid* pyr, int first_slot, int n_slots, const uint8_t* packed);
/* n_slots level-0 images (back to back on the host) in one strided transfer, then the coarser levels of all of them
 * on the device: 4 launches for the whole batch, and only level 0 (75 % of the pyramid bytes) crosses the link */
int svo_hip_pyramid_upload_level0_batch_and_build(svo_hip_pyramid* pyr, int first_slot, int n_slots,
                                                  const uint8_t* level0_packed);
int svo_hip_pyramid_info(const svo_hip_pyramid* pyr, int* width, int* height, int* n_levels, int* batch,
                         size_t* pyr_bytes, void** base_dev);

/* ---- SparseImgAlign (I/sparse_img_align.h:33-79, sparse_img_align.cpp:51-308,
 *      I/nlls_solver_impl.hpp:25-100) ------------------------------------------------------ */
typedef struct {
  int max_level, min_level;   /* SparseImgAlign ctor args n_levels / min_level (:29-41)        */
  int n_iter;                 /* n_iter_ (:35)                                                 */
  double eps;                 /* eps_ = 1e-6 (:40)                                             */
  int early_stop;             /* 1: reference Gauss-Newton exits (error increase, |x|<=eps);
                                 0: fixed work, exactly n_iter evaluations per level           */
} svo_hip_sia_params;

typedef struct {
  double T_cur_w[7];          /* cur_frame_->T_f_w_ after run() (:89)                          */
  uint64_t n_tracked;         /* return value of run(): n_meas_/patch_area_ (:91)              */
  double H[36];               /* H_ of the last evaluation: getInformationMatrix()             */
  double chi2;                /* getChi2()                                                      */
  int stop;                   /* stop_                                                          */
  int iters[SVO_HIP_MAX_LEVELS];   /* residual evaluations per pyramid level                    */
  uint64_t n_precompute_patches;   /* algorithmic work counters: sum over levels    */
  uint64_t n_residual_patches;     /* and over evaluations of patches actually accumulated      */
} svo_hip_sia_result;

/* A solver for `batch` independent frame pairs with up to max_features features each. */
int svo_hip_sia_create(svo_hip_ctx* ctx, int batch, int max_features, svo_hip_sia** out);
int svo_hip_sia_destroy(svo_hip_sia* sia);
/* slot s of the solver aligns ref->slot s against cur->slot s (pyramids must outlive the solver use) */
int svo_hip_sia_set_frames(svo_hip_sia* sia, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur);
/* Flattened ref_frame->fts_ in list order (sparse_img_align.cpp:116-118): level-0 pixel px[n][2],
 * unit bearing f[n][3], world position of the feature's point pos[n][3], has_point[n] (point != NULL). */
int svo_hip_sia_upload_features(svo_hip_sia* sia, int slot, int n, const double* px, const double* f,
                                const double* pos, const uint8_t* has_point);
/* ref_frame->T_f_w_, the initial cur_frame->T_f_w_ and the camera of the pair */
int svo_hip_sia_upload_poses(svo_hip_sia* sia, int slot, const svo_hip_camera* cam,
                             const double T_ref_w[7], const double T_cur_w_init[7]);
/* Only patches [n*rank/world, n*(rank+1)/world) of every frame are evaluated by this process;
 * the per-frame sums must then be all-reduced across ranks between accumulate and solve_update (step-wise entry
 * points).  svo_hip_sia_run returns SVO_HIP_ERR_STATE while world != 1: a whole solve over one shard without the
 * exchange would be a different problem. */
int svo_hip_sia_set_shard(svo_hip_sia* sia, int rank, int world);

/* ---- multi-GPU exchange: the reference has none; these entries let the C++ host shard the path ----
 * A communicator binds a context (its stream) to a rank of a group.  Transports:
 *   RCCL over xGMI: either the library creates the communicator from a 128-byte ncclUniqueId that rank 0 obtained
 *     with svo_hip_comm_unique_id and the application distributed (MPI, a file, a socket ...), or it adopts an existing
 *     ncclComm_t (svo_hip_comm_from_nccl; the application keeps ownership).  librccl is resolved at run time.
 *   host-staged exchange through a POSIX shared-memory segment `name` ("/..."; unique per group): for ranks that
 *     share one device or have no peer path (bring-up, tests).  slot_bytes = largest message of one rank.  Blocks the
 *     calling thread at every exchange.
 * Both give every rank bitwise the same all-reduce result, so the ranks' Gauss-Newton decisions stay in lock-step. */
typedef struct svo_hip_comm svo_hip_comm;
int svo_hip_comm_unique_id(void* id128);
int svo_hip_comm_create_rccl(svo_hip_ctx* ctx, const void* id128, int rank, int world, svo_hip_comm** out);
int svo_hip_comm_from_nccl(svo_hip_ctx* ctx, void* nccl_comm, int rank, int world, svo_hip_comm** out);
int svo_hip_comm_create_shm(svo_hip_ctx* ctx, const char* name, int rank, int world, size_t slot_bytes, svo_hip_comm** out);
int svo_hip_comm_destroy(svo_hip_comm* comm);
int svo_hip_comm_info(const svo_hip_comm* comm, int* rank, int* world, int* kind /* 0 RCCL, 1 shared memory */);
/* the rank count the transport itself reports (ncclCommCount / the segment header), not the creation argument */
int svo_hip_comm_count(const svo_hip_comm* comm, int* count);

/* SparseImgAlign::run with every frame's patches split over the ranks of `comm` (BASELINE config C3's variant): each
 * rank evaluates patches [n*rank/world, n*(rank+1)/world) of every slot, ONE all-reduce of n_slots x
 * SVO_HIP_REDUCE_DOUBLES doubles per Gauss-Newton step on the context stream, then the identical solve on every rank.
 * Every rank must hold the same features, poses and pyramids and call this with the same arguments; all ranks end
 * with the same result (svo_hip_sia_download).  comm must have been created on the solver's context (one stream for
 * kernels and collective).  The shard is in force for this call only: a shard set with svo_hip_sia_set_shard is back
 * in place when it returns. */
int svo_hip_sia_run_sharded(svo_hip_sia* sia, svo_hip_comm* comm, int n_slots, const svo_hip_sia_params* prm);
/* Opt-in: replay the per-level launch sequence of svo_hip_sia_run_sharded (level_begin + n_iter x {accumulate,
 * all-reduce, solve_update}) from one HIP graph per pyramid level, captured at the first call of a configuration (RCCL
 * transport only).  Saves host launch time, not device time. */
int svo_hip_sia_set_sharded_graph(svo_hip_sia* sia, int enable);

/* run(): the whole coarse-to-fine solve for slots [0, n_slots), enqueued on the stream with no
 * host round trip (the default, Gauss-Newton; with SVO_HIP_SIA_OPT_METHOD / _SCALE_ESTIMATOR / _CHI2 set the call looks
 * at the frames' state between rounds of evaluations and so waits for the device: see those options).  Poses restart
 * from the uploaded initial poses on every call. */
int svo_hip_sia_run(svo_hip_sia* sia, int n_slots, const svo_hip_sia_params* prm);
/* blocks until the stream is idle, then copies the result of one slot */
int svo_hip_sia_download(svo_hip_sia* sia, int slot, svo_hip_sia_result* out);
/* all slots at once (out[n_slots]) */
int svo_hip_sia_download_all(svo_hip_sia* sia, int n_slots, svo_hip_sia_result* out);

/* The same solve in steps, for callers that exchange the normal equations between devices:
 *   begin; for level = max..min { level_begin(level); n_iter x { accumulate; [all-reduce]; solve_update } } finish
 * accumulate leaves SVO_HIP_REDUCE_DOUBLES doubles per slot in the reduce buffer. */
int svo_hip_sia_begin(svo_hip_sia* sia, int n_slots, const svo_hip_sia_params* prm);
int svo_hip_sia_level_begin(svo_hip_sia* sia, int level);
int svo_hip_sia_accumulate(svo_hip_sia* sia);
int svo_hip_sia_solve_update(svo_hip_sia* sia);
int svo_hip_sia_finish(svo_hip_sia* sia);
/* device address of the reduce buffer ([batch][SVO_HIP_REDUCE_DOUBLES] doubles) */
int svo_hip_sia_reduce_buffer(svo_hip_sia* sia, void** dev_ptr, size_t* n_doubles);
/* use a caller-owned device buffer instead (e.g. a torch tensor that RCCL all-reduces in place) */
int svo_hip_sia_set_reduce_buffer(svo_hip_sia* sia, void* dev_ptr);
/* Tuning / diagnostic switches of ONE solver object (the library reads no environment variable and keeps no
 * process-wide switch: two host threads with two solvers do not see each other's settings).  0 = automatic unless
 * stated otherwise. */
#define SVO_HIP_SIA_OPT_MODE 0          /* SVO_HIP_SIA_MODE_AUTO, or SVO_HIP_SIA_MODE_STREAM: svo_hip_sia_run always uses the streaming kernels */
#define SVO_HIP_SIA_OPT_WAVES 1         /* fused kernel: waves per frame pair, 0 (automatic), 4 or 8 */
#define SVO_HIP_SIA_OPT_CHUNKS 2        /* streaming residual kernel: workgroups per frame, 0 (automatic) .. 64 */
#define SVO_HIP_SIA_OPT_EXTRA_LDS 3     /* fused kernel: waves with a third tile in LDS, -1 (automatic) .. 3 */
#define SVO_HIP_SIA_OPT_OLD_TILES 4     /* fused kernel: tiles of the older wave of a SIMD, 0 (automatic) .. 6 */
#define SVO_HIP_SIA_OPT_ARITH 5         /* fused kernel: SVO_HIP_SIA_ARITH_EXACT (default: the reference's arithmetic), _MOMENTS_F32 or _FAST (opt-in) */
#define SVO_HIP_SIA_OPT_METHOD 6          /* NLLSSolver::method_ (I/nlls_solver.h:46): SVO_HIP_SIA_METHOD_GAUSS_NEWTON (default) or _LEVENBERG_MARQUARDT */
#define SVO_HIP_SIA_OPT_SCALE_ESTIMATOR 7 /* setRobustCostFunction's first argument (:47): SVO_HIP_SIA_SCALE_UNIT (default: no weights), _TDIST, _MAD, _NORMAL */
#define SVO_HIP_SIA_OPT_WEIGHT_FUNCTION 8 /* ... and its second (:48): SVO_HIP_SIA_WEIGHT_UNIT (default), _TDIST, _TUKEY, _HUBER */
#define SVO_HIP_SIA_OPT_CHI2 9            /* SVO_HIP_SIA_CHI2_PER_PATCH (default) or _REFERENCE_ORDER, see below */
#define SVO_HIP_SIA_OPT_REDUCTION 10      /* fused kernel: SVO_HIP_SIA_REDUCTION_PER_WAVE (default) or _TILE_ORDER (opt-in), see below */
#define SVO_HIP_SIA_MODE_AUTO 0
#define SVO_HIP_SIA_MODE_STREAM 1
/* Arithmetic levels of the fused kernel.  At every level the image math is the reference's f32, pixel choice, projection,
 * H_ (formed once per level from the patches' gradient sums), normal equations, solve and the Gauss-Newton control flow are
 * unchanged: H_, the tracked-patch count and -- on every scene tested -- the iteration counts are bit for bit the same
 * from one level to the other, for the same batch.  (What a frame's bits owe to the OTHER frames of its batch is a matter of
 * the grouping of the sums, not of the arithmetic level: SVO_HIP_SIA_OPT_REDUCTION below.  In the default grouping H_, Jres_
 * and chi2 depend in their last bits on the batch's largest frame and size at every level; in _TILE_ORDER, which exists for
 * EXACT only, nothing does.)
 * EXACT (the default; round 4 shipped MOMENTS_F32 as the default, round 5 took that back: every caller that sets nothing --
 *   the drop-in SparseImgAlign::run binding included -- gets the reference's arithmetic): the reference's arithmetic
 *   statement by statement -- uncontracted f32 interpolation, residual products and Jacobian moments in f64
 *   (sparse_img_align.cpp:238-279): with a fixed evaluation count poses agree with the CPU path to ~1e-13 ... 6e-9 rad.
 * MOMENTS_F32 (opt-in, pays only in launches of thousands of frame pairs): EXACT's residuals and chi2; the 16 products
 *   dx*res and dy*res of a patch are
 *   accumulated in f32 (one fused rounding per term) and widened once per patch, instead of exactly in f64 -- three
 *   conversions and two f64 operations per pixel less, the solve runs ~7 % faster.  Poses agree with the CPU path to
 *   ~3e-8 rad / 6e-8 m with a fixed evaluation count (tests assert 1e-7 against EXACT) and, with the reference's own exits
 *   -- where the f32 chi2 summation order already decides -- exactly as well as EXACT does (5e-8 rad); the reference's own
 *   translation units built for arm64 move by 1.4e-8 rad.  north_star allows 1e-4 rad / 1e-3 m.
 * FAST: additionally the bilinear sum contracted (one product + three fused multiply-adds) and chi2 summed with fused
 *   multiply-adds: ~10 % faster than EXACT, poses ~2e-8 rad from the CPU path.
 * Applies to the fused kernel (svo_hip_sia_run); the streaming / step-wise / sharded paths and svo_hip_tracker's own
 * solver always use EXACT. */
#define SVO_HIP_SIA_ARITH_EXACT 0
#define SVO_HIP_SIA_ARITH_FAST 1
#define SVO_HIP_SIA_ARITH_MOMENTS_F32 2
/* The other branches of vk::NLLSSolver<6,SE3> that SparseImgAlign inherits (I/nlls_solver.h:46-48; no caller in the
 * reference enables them -- frame_handler_mono.cpp:186-187,331-332 construct with GaussNewton and set no robust cost).
 * The values are the reference's enumerators.
 *   METHOD _LEVENBERG_MARQUARDT: optimizeLevenbergMarquardt (I/nlls_solver_impl.hpp:102-227) as SparseImgAlign::run drives
 *     it (mu_ = 0.1 at every level, S/sparse_img_align.cpp:74), with what the reference does around it: n_meas_ is not
 *     cleared before a level's first evaluation (so chi2_ starts low on every level but the first), stop_ survives into the
 *     next level, H_ is the DAMPED matrix of the last trial, params.early_stop is ignored and n_iter bounds the outer
 *     iterations (up to 5 trials each).  result.iters counts evaluations; a trial costs one, not the reference's two: the
 *     sums of the evaluation at an accepted pose are kept and are the next linearisation.
 *   SCALE_ESTIMATOR / WEIGHT_FUNCTION: setRobustCostFunction (:229-281).  _SCALE_UNIT switches the weights off whatever
 *     the weight function (as there).  The scale is estimated at a level's first pose when iter_ of the level before ended
 *     at 0, i.e. normally once per run (S/sparse_img_align.cpp:281-283); the estimators are evaluated in f32 in the order
 *     of the reference's errors vector (TDist and Normal sum sequentially; MAD selects the element nth_element leaves at
 *     size/2; Normal reproduces std::accumulate's int seed), so scale_ is the reference's bit for bit.
 * Both run over the streaming kernels (svo_hip_sia_last_run_mode 0), one launch pair per evaluation, and svo_hip_sia_run
 * looks at the frames' state after every sixth evaluation of a level (the number of trials is data dependent): unlike the
 * default path the call waits for the device.  The step-wise and sharded entry points
 * refuse a solver that has either set (SVO_HIP_ERR_STATE).  chi2 is added up in the reference's order on these paths
 * (SVO_HIP_SIA_OPT_CHI2 below): Levenberg-Marquardt accepts or rejects a trial on the sign of a chi2 difference that is
 * often a few units in the last place. */
/* CHI2: how the residuals' squares are added up.  The reference adds every pixel of every patch, in list order, into ONE
 * f32 (float chi2 ... chi2 += res*res*weight, S/sparse_img_align.cpp:207,266) and decides on that sum whether an iteration
 * increased the error (I/nlls_solver_impl.hpp:62).  _PER_PATCH (default; the fused kernel, the streaming and sharded paths,
 * the tracking chain): f32 within a patch, f64 over the patches -- a better sum, and the only one that parallelises; when two
 * successive values differ by a few units in the last place of the reference's f32 sum, the error-increase exit can fall
 * one iteration earlier or later than in the reference (poses then differ by < 2e-5 rad / 5e-5 m on the scenes tested).
 * _REFERENCE_ORDER: the squares go to memory and are added in the reference's order: chi2_ is the reference's bit
 * for bit and every exit falls where the reference's does.  Costs ~25 us per evaluation at 200 patches (one lane) and ~60 us
 * at 2000 (a workgroup: svo_hip_ordered_sum_f32_dev below) on top of the streaming kernels (svo_hip_sia_last_run_mode 0);
 * Levenberg-Marquardt and the robust costs always use it. */
#define SVO_HIP_SIA_CHI2_PER_PATCH 0
#define SVO_HIP_SIA_CHI2_REFERENCE_ORDER 1
/* SVO_HIP_SIA_OPT_REDUCTION: how the fused kernel groups the 29 sums of an evaluation (21 entries of H_, 6 of Jres_, chi2,
 * n_meas).  Everything before the sums is per patch or per 64-patch tile and everything after them is a function of the sums,
 * so the grouping is the only thing through which the other frame pairs of a launch can reach a frame's result.
 * _PER_WAVE (default): a wave adds the lane values of all the tiles it owns, reduces once, and the waves are added in fixed
 *   order.  Which tiles a wave owns is the kernel shape, chosen per launch from the launch's largest frame and its number of
 *   pairs (and by SVO_HIP_SIA_OPT_WAVES / _OLD_TILES): the last bits of a frame's H_, Jres_ and chi2 -- and through them of
 *   its pose; on a borderline frame an iteration count -- depend on the company the frame is launched in.  Reproducible run
 *   to run for the same batch.
 * _TILE_ORDER (opt-in): every tile is reduced over its 64 lanes on its own and the tiles' totals are added in ascending
 *   tile order, in f64, by one wave.  Every field of svo_hip_sia_result is then a function of the frame pair alone: equal
 *   bytes whatever the batch size, the other frames, the slot, the kernel shape and the diagnostic shape options
 *   (tests/test_gpu_sia_batch_invariance.py).  The results differ from _PER_WAVE's in the last bits and meet the same
 *   tolerances against the reference.  Measured cost (profiles/HISTORY.md): C1 -- 2000 patches, 4096 pairs per launch, fixed
 *   work -- 21.16 against 19.08 ms per step, a time ratio of 1.11 (193.6 k against 214.7 k frames/s); by kernel shape between
 *   0.88 and 1.11 (tools/reduction_shapes.py); the lone tracking chain +0.7 % per frame, inside its run-to-run spread.
 *   Besides the sums, the mode's kernels take ONE form of the outside-the-image correction of a tile's H row in every shape:
 *   the default kernels for more than 2048 patches use another form than the smaller shapes, which is a second way the
 *   largest frame of a batch reaches the others' last bits in the default mode.
 *   svo_hip_sia_run must take the fused kernel then.  Where it cannot it fails with SVO_HIP_ERR_STATE and runs nothing:
 *   SVO_HIP_SIA_MODE_STREAM, a frame of more than 2816 patches, Levenberg-Marquardt, a robust cost,
 *   SVO_HIP_SIA_CHI2_REFERENCE_ORDER (the streaming kernels group by workgroups per frame, which follow the batch size) and
 *   an arithmetic level other than SVO_HIP_SIA_ARITH_EXACT (the mode's kernels exist for that level only).
 *   The step-wise entry points (svo_hip_sia_begin ... _finish) and svo_hip_sia_run_sharded always run the streaming kernels
 *   and are not affected by this option. */
#define SVO_HIP_SIA_REDUCTION_PER_WAVE 0
#define SVO_HIP_SIA_REDUCTION_TILE_ORDER 1
#define SVO_HIP_SIA_METHOD_GAUSS_NEWTON 0
#define SVO_HIP_SIA_METHOD_LEVENBERG_MARQUARDT 1
#define SVO_HIP_SIA_SCALE_UNIT 0
#define SVO_HIP_SIA_SCALE_TDIST 1
#define SVO_HIP_SIA_SCALE_MAD 2
#define SVO_HIP_SIA_SCALE_NORMAL 3
#define SVO_HIP_SIA_WEIGHT_UNIT 0
#define SVO_HIP_SIA_WEIGHT_TDIST 1
#define SVO_HIP_SIA_WEIGHT_TUKEY 2
#define SVO_HIP_SIA_WEIGHT_HUBER 3
int svo_hip_sia_set_option(svo_hip_sia* sia, int option, int value);
/* The f32 sum of n values in index order, rounded exactly as `float s = 0; for (k...) s += x[k];` rounds it -- the form
 * of the reference's chi2 (S/sparse_img_align.cpp:207,266) and of its scale estimators' sums (S/robust_cost.cpp:53-60,83-85)
 * -- by one 1024-thread workgroup instead of a chain of n dependent additions (android_svo_amd/csrc/svo_ordered_sum.h: inside
 * a binade a non-negative addition depends on its predecessors through the parity of the running sum only; sequences of up
 * to 4096 values, and any stretch with a negative, infinite or NaN value, are added by one lane).  1.0 ns per value for long
 * sequences, 62 us for 32 000 values, against 5 ns per value for the one-lane chain (tools/ordered_sum_probe.py).  Enqueued on the context's stream.  What
 * SVO_HIP_SIA_CHI2_REFERENCE_ORDER, Levenberg-Marquardt and the robust costs use. */
int svo_hip_ordered_sum_f32_dev(svo_hip_ctx* ctx, const float* vals_dev, size_t n, float* out_dev);
/* scale_, mu_ and nu_ of one slot as the last svo_hip_sia_run with Levenberg-Marquardt or a robust cost left them
 * (blocks until the stream is idle; SVO_HIP_ERR_STATE when no such run has been made or `slot` was not one of its frames) */
int svo_hip_sia_solver_state(svo_hip_sia* sia, int slot, float* scale, double* mu, double* nu);

/* Which implementation the last svo_hip_sia_run used: 1 = the fused kernel (one workgroup per frame pair,
 * interpolated reference patches in LDS / L2-resident memory, whole coarse-to-fine loop in one launch; chosen
 * when every frame has at most 2816 features and no patch shard is set; launches with at least two frame pairs
 * per compute unit and at most 1024 features per frame use its 4-wave shape, two pairs per compute unit),
 * 0 = the streaming kernels (one launch per Gauss-Newton evaluation; always used by the step-wise entry
 * points).  svo_hip_sia_set_option(SVO_HIP_SIA_OPT_MODE, SVO_HIP_SIA_MODE_STREAM) forces 0.  In a batch that holds
 * frames with fewer than 16 patches those frames take the entry-by-entry Hessian rows a rank-deficient system needs
 * (chosen per workgroup); the other frames' results are bit for bit what they are without such company.  With the
 * default SVO_HIP_SIA_REDUCTION_PER_WAVE a frame's result does depend, in the last bits, on the kernel shape, i.e. on the
 * largest frame of the batch and on the number of pairs; with SVO_HIP_SIA_REDUCTION_TILE_ORDER it depends on nothing but
 * the frame pair (SVO_HIP_SIA_OPT_REDUCTION above). */
int svo_hip_sia_last_run_mode(svo_hip_sia* sia, int* mode);
/* Optional timing of the two heavy kernels with HIP events recorded on the context stream around
 * each launch (precompute: one per level; residual: one per Gauss-Newton evaluation; in fused mode the single
 * launch of a run is reported in the `residual` slot).
 * get_profile synchronises, returns the summed device time and launch counts since the last call
 * and resets the counters. */
int svo_hip_sia_set_profiling(svo_hip_sia* sia, int enable);
int svo_hip_sia_get_profile(svo_hip_sia* sia, double* residual_ms, uint64_t* residual_launches,
                            double* precompute_ms, uint64_t* precompute_launches);
/* cached reference patches / per-patch Jacobian records of one slot, for kernel-level tests (filled by the
 * streaming kernels, i.e. after the step-wise entry points or a run in SVO_HIP_SIA_MODE_STREAM):
 * ref_patch[n][16] f32, dx[n][16] f32, dy[n][16] f32, visible[n] u8 (any may be NULL).  Returns SVO_HIP_ERR_STATE when
 * the last svo_hip_sia_run used the fused kernel (it keeps no per-pixel caches in memory). */
int svo_hip_sia_download_caches(svo_hip_sia* sia, int slot, float* ref_patch, float* dx, float* dy,
                                uint8_t* visible);
/* The same quantities as the FUSED kernel forms them at one pyramid level (it keeps them in LDS / L2-resident memory as
 * 32 interpolated values per patch and never writes per-pixel caches): recomputed by a kernel that shares the fused
 * kernel's device functions for the feature position, the weights and the interpolation, for kernel-level tests against
 * precomputeReferencePatches (sparse_img_align.cpp:144-175).  valid[n]: patches inside the level image with a point;
 * rows of other patches are not written.  Overwrites the streaming kernels' cache arrays of the slot. */
int svo_hip_sia_download_fused_patches(svo_hip_sia* sia, int slot, int level, float* ref_patch, float* dx, float* dy,
                                       uint8_t* valid);
/* Test support as well: Jres_ [6] and x_ [6] of the slot's last Gauss-Newton evaluation, which svo_hip_sia_result does not
 * carry (tests/test_gpu_fused_window_paths.py holds them to recorded bits).  Blocks like svo_hip_sia_download. */
int svo_hip_sia_download_last_step(svo_hip_sia* sia, int slot, double* Jres6, double* x6);

/* ---- feature_alignment::align2D (I/feature_alignment.h:40-47, feature_alignment.cpp:154-282) */
/* n independent 8x8 patches refined on level `level` of cur->slot: ref_patch_with_border
 * [n][100] u8, ref_patch [n][64] u8 (NULL: the interior of the bordered patch, which is how every caller of the
 * reference fills it, matcher.cpp:138-147), px [n][2] f64 in/out (level coordinates), converged [n] u8,
 * iters [n] i32 (iterations executed; may be NULL).  All pointers are device pointers; the patch arrays must be
 * 4-byte aligned (the reference's are 16-byte aligned members of Matcher).
 * One lane per patch walks the 64 pixels in the reference's order: `converged` and px equal the CPU path's bit for
 * bit. */
int svo_hip_align2d_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* cur, int slot, int level, int n,
                              const uint8_t* ref_patch_with_border_dev, const uint8_t* ref_patch_dev,
                              int n_iter, double* px_dev, uint8_t* converged_dev, int32_t* iters_dev);
/* host-buffer convenience form (copies in, runs, copies out, synchronises) */
int svo_hip_align2d_batch(svo_hip_ctx* ctx, const svo_hip_pyramid* cur, int slot, int level, int n,
                          const uint8_t* ref_patch_with_border, const uint8_t* ref_patch, int n_iter,
                          double* px, uint8_t* converged, int32_t* iters);

/* feature_alignment::align1D (I/feature_alignment.h:30-38, feature_alignment.cpp:35-152): n patches that may only
 * move along dir[n][2] (f32, e.g. the epipolar direction); h_inv[n] f64 out (may be NULL).  Device pointers. */
int svo_hip_align1d_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* cur, int slot, int level, int n,
                              const uint8_t* ref_patch_with_border_dev, const float* dir_dev, int n_iter,
                              double* px_dev, uint8_t* converged_dev, double* h_inv_dev, int32_t* iters_dev);

/* ---- Matcher::findMatchDirect over a batch (I/matcher.h:108-111, matcher.cpp:156-202) ----------
 * n (map point, reference feature) pairs against frame cur->cur_slot: frame test of the reference feature,
 * depth = |ref_pos - pt_pos|, warp::getWarpMatrixAffine, getBestSearchLevel, warpAffine, then align2D
 * (align1D along A*grad for EDGELET reference features).  Point::getCloseViewObs and the reprojector's
 * first-success-per-cell policy stay on the host: the caller passes the reference feature it chose.
 * ref holds the n_kf keyframe pyramids (slot k <-> T_ref_w_dev[k][7]); per item: kf_slot, px_ref[2], f_ref[3],
 * level_ref, pt_pos[3], optional edgelet flag + grad[2]; px_cur[n][2] in (estimate) / out, success[n] u8,
 * search_level[n] (may be NULL).  Device pointers except T_cur_w. */
int svo_hip_match_direct_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur,
                                   int cur_slot, const svo_hip_camera* cam, int n_kf, const double* T_ref_w_dev,
                                   const double T_cur_w[7], int n, const int32_t* kf_slot_dev,
                                   const double* px_ref_dev, const double* f_ref_dev, const int32_t* level_ref_dev,
                                   const double* pt_pos_dev, const uint8_t* edgelet_dev, const double* grad_dev,
                                   int n_pyr_levels, int align_max_iter, double* px_cur_dev, uint8_t* success_dev,
                                   int32_t* search_level_dev);

/* The cell loop of Reprojector::reprojectMap (I/reprojector.h:57-59, reprojector.cpp:149-166 with reprojectCell
 * :180-241) on host buffers: candidates bucketed per grid cell in trial order (cell.sort(pointQualityComparator)
 * applied by the caller); candidates of cell c = [cell_offset[c], cell_offset[c+1]).  All candidates are matched in
 * one batch, then the reference's serial policy is replayed (first success per cell wins, candidates behind the
 * winner untouched, stop once n_matches exceeds max_fts = Config::maxFts()).  deleted[i] <=> the point's type is
 * TYPE_DELETED.  Outputs: tried[i] / matched[i] (what the caller needs for the point bookkeeping of :202-215),
 * px_cur[i] and search_level[i] of the visited candidates, cell_winner[c] (candidate index or -1), n_matches_,
 * n_trials_. */
int svo_hip_reproject_cells(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, const svo_hip_pyramid* cur, int cur_slot,
                            const svo_hip_camera* cam, int n_kf, const double* T_kf_w, const double T_cur_w[7], int n_cells,
                            const int32_t* cell_offset, const int32_t* kf_slot, const double* px_ref, const double* f_ref,
                            const int32_t* level_ref, const double* pt_pos, const uint8_t* edgelet, const double* grad,
                            const uint8_t* deleted, double* px_cur, int max_fts, int n_pyr_levels, int align_max_iter,
                            uint8_t* tried, uint8_t* matched, int32_t* search_level, int32_t* cell_winner,
                            uint64_t* n_matches, uint64_t* n_trials);

/* ---- DepthFilter (I/depth_filter.h:36-166, depth_filter.cpp:237-416; matcher.cpp:207-355) -- */
/* static DepthFilter::updateSeed over n seeds (depth_filter.cpp:368-391): SoA device arrays */
int svo_hip_update_seed_batch_dev(svo_hip_ctx* ctx, int n, const float* x_dev, const float* tau2_dev,
                                  float* a_dev, float* b_dev, float* mu_dev, const float* z_range_dev,
                                  float* sigma2_dev);
/* static DepthFilter::computeTau over n (f, z) pairs sharing one T_ref_cur (depth_filter.cpp:396-416) */
int svo_hip_compute_tau_batch_dev(svo_hip_ctx* ctx, int n, const double T_ref_cur[7], const double* f_dev,
                                  const double* z_dev, double px_error_angle, double* tau_dev);

typedef struct {
  int n_pyr_levels;                  /* Config::nPyrLevels() (config.cpp:59: 3)                   */
  int align_max_iter;                /* Matcher::Options::align_max_iter (I/matcher.h:86: 10)      */
  int max_epi_search_steps;          /* Matcher::Options::max_epi_search_steps (I/matcher.h:88: 1000) */
  double seed_convergence_sigma2_thresh;   /* DepthFilter::Options (I/depth_filter.h:85: 100.0)    */
} svo_hip_df_params;

/* per-seed outcome of one updateSeeds pass (depth_filter.cpp:250-340) */
#define SVO_HIP_SEED_BEHIND 0
#define SVO_HIP_SEED_NOT_IN_FRAME 1
#define SVO_HIP_SEED_NO_MATCH 2
#define SVO_HIP_SEED_UPDATED 3
#define SVO_HIP_SEED_CONVERGED 4
#define SVO_HIP_SEED_NAN 5
#define SVO_HIP_SEED_ERASED (-1)   /* seed batches only: the seed had left the list before this pass (nothing was computed) */

/* DepthFilter::updateSeeds for n seeds created in keyframe ref->ref_slot, measured in frame
 * cur->cur_slot: visibility test, Matcher::findEpipolarMatchDirect (epipolar ZMSSD search +
 * align2D + triangulation), computeTau, updateSeed, convergence test.  SoA device arrays:
 * px[n][2] f64, f[n][3] f64, level[n] i32 (Feature px/f/level), a,b,mu,sigma2 in/out f32, z_range f32;
 * outputs status[n] i32, z[n] f64, xyz_world[n][3] f64 (valid when converged), the work
 * counters n_zmssd[n], n_align_iters[n] i32, and the matcher's public results of the seed's call:
 * px_cur[n][2] f64 = Matcher::px_cur_ (level-0 pixel of the match, matcher.cpp:345; valid where status >=
 * SVO_HIP_SEED_UPDATED, NaN elsewhere) -- what updateSeeds passes to feature_detector_->setGridOccpuancy on
 * keyframes (depth_filter.cpp:302-306) -- and search_level[n] i32 = Matcher::search_level_ (-1 for seeds that
 * never reached the matcher).  Any output except status may be NULL. */
int svo_hip_depth_filter_update_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int ref_slot,
                                    const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam,
                                    const double T_ref_w[7], const double T_cur_w[7], int n,
                                    const double* px_dev, const double* f_dev, const int32_t* level_dev,
                                    float* a_dev, float* b_dev, float* mu_dev, const float* z_range_dev,
                                    float* sigma2_dev, const svo_hip_df_params* prm, int32_t* status_dev,
                                    double* z_dev, double* xyz_world_dev, int32_t* n_zmssd_dev,
                                    int32_t* n_align_iters_dev, double* px_cur_dev, int32_t* search_level_dev);

/* Matcher::findEpipolarMatchDirect over n reference features (I/matcher.h:113-121, matcher.cpp:207-355) with the
 * depth interval given by the caller: depth_est_min_max[3][n] f64 = d_estimate[n], d_min[n], d_max[n].  Outputs:
 * ok[n] u8 (the return value), depth[n] f64 (the `depth` out-parameter), and the public members the call leaves
 * behind: px_cur[n][2] (px_cur_; NaN when the alignment failed), search_level[n] (search_level_), epi_length[n]
 * (epi_length_), plus the work counters.  Any output except ok may be NULL.  Device pointers. */
int svo_hip_epipolar_match_batch_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int ref_slot,
                                     const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam,
                                     const double T_ref_w[7], const double T_cur_w[7], int n, const double* px_dev,
                                     const double* f_dev, const int32_t* level_dev,
                                     const double* depth_est_min_max_dev, const svo_hip_df_params* prm,
                                     uint8_t* ok_dev, double* depth_dev, double* px_cur_dev, int32_t* search_level_dev,
                                     double* epi_length_dev, int32_t* n_zmssd_dev, int32_t* n_align_iters_dev);

/* Converged seeds of a batch as packed records {seed id = id_offset + index, mu, sigma2, x, y, z} (f64[6]), in seed
 * order, plus their number: the payload of the multi-GPU gather of SURVEY 8e (and of the seed_converged callbacks,
 * depth_filter.cpp:313-329).  records_dev must hold n records. */
int svo_hip_seed_compact_converged_dev(svo_hip_ctx* ctx, int n, long long id_offset, const int32_t* status_dev,
                                       const float* mu_dev, const float* sigma2_dev, const double* xyz_world_dev,
                                       double* records_dev, int32_t* count_dev);

/* The exchange step of the seed-sharded depth filter (BASELINE config C4): this rank's converged seeds (packed as
 * above, clamped to `cap` records) and every other rank's, plus the per-rank counts: records_all[world][cap][6] f64,
 * counts_all[world] i32 (a count above cap means that rank had more: call again with a larger cap).  Two fixed-size
 * all-gathers on the context stream. */
int svo_hip_seed_gather_converged_dev(svo_hip_ctx* ctx, svo_hip_comm* comm, int n, long long id_offset,
                                      const int32_t* status_dev, const float* mu_dev, const float* sigma2_dev,
                                      const double* xyz_world_dev, int cap, double* records_all_dev,
                                      int32_t* counts_all_dev);

/* diagnostic: HIP events around the four stages (geometry, search, align, finalize) of every following depth-filter pass
 * of this context; svo_hip_df_get_profile waits for the last pass and returns its stage durations in microseconds */
int svo_hip_df_set_profiling(svo_hip_ctx* ctx, int enable);
int svo_hip_df_get_profile(svo_hip_ctx* ctx, double stage_us[4]);

/* ---- device-resident seeds: the seeds DepthFilter::initializeSeeds creates for one keyframe (depth_filter.cpp:129-151)
 * live on the device from their creation to their end.  The host uploads a batch ONCE (Feature px / f / level and the
 * Seed constructor's a, b, mu, z_range, sigma2); every frame only the two poses go down (svo_hip_seed_batch_update_async)
 * and only the seeds whose outcome the host must act on come back (svo_hip_seed_batch_collect): seeds that converged
 * (:310-331: new Point at xyz_world, seed_converged_cb(point, sigma2), erase) or turned NaN (:333-337: erase) -- the
 * device stops updating them, as the list erase does -- and, when report_updated is set (the frame is a keyframe,
 * :302-306), every updated seed with its Matcher::px_cur_ for feature_detector_->setGridOccpuancy.  Events are ordered
 * by seed index = list order, so callbacks happen in the reference's order.  Seeds the HOST erases (removeKeyframe,
 * age-out of a part of a batch) are reported with svo_hip_seed_batch_erase.  svo_hip_seed_batch_download returns the
 * current state of every seed for getSeeds() / getSeedsCopy().  One batch belongs to one context (one host thread). */
typedef struct svo_hip_seed_batch svo_hip_seed_batch;
typedef struct {
  int32_t index;            /* position in the batch = creation order of the keyframe's seeds */
  int32_t status;           /* SVO_HIP_SEED_CONVERGED, SVO_HIP_SEED_NAN or (report_updated) SVO_HIP_SEED_UPDATED */
  float mu, sigma2;         /* Seed::mu / Seed::sigma2 after the update */
  double xyz_world[3];      /* converged seeds: ref.T_f_w_.inverse() * (f / mu) (:313) */
  double px_cur[2];         /* Matcher::px_cur_ (level-0 pixel in the current frame) */
} svo_hip_seed_event;
int svo_hip_seed_batch_create(svo_hip_ctx* ctx, int n, const double* px, const double* f, const int32_t* level,
                              const float* a, const float* b, const float* mu, const float* z_range, const float* sigma2,
                              svo_hip_seed_batch** out);                     /* host arrays, uploaded once */
int svo_hip_seed_batch_destroy(svo_hip_seed_batch* batch);
int svo_hip_seed_batch_size(const svo_hip_seed_batch* batch, int* n, int* n_alive);     /* n_alive: as of the last collect */
/* enqueue one updateSeeds pass of the batch against cur->cur_slot on the context stream (returns at once): the group call
 * below with one batch */
int svo_hip_seed_batch_update_async(svo_hip_seed_batch* batch, const svo_hip_pyramid* ref, int ref_slot,
                                    const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam,
                                    const double T_ref_w[7], const double T_cur_w[7], const svo_hip_df_params* prm,
                                    int report_updated);
/* The same pass over SEVERAL batches of one context -- the seeds of every keyframe a frame updates (the loop of
 * depth_filter.cpp:248-340 walks them all) -- as ONE set of launches: batch k against keyframe slot ref_slots[k] of `ref`
 * with pose T_ref_w[7 * k .. 7 * k + 6].  Results per batch are bit-identical to n_batches calls of
 * svo_hip_seed_batch_update_async; what changes is the cost when the batches are small (a few hundred seeds each is what
 * the reference's detector yields per keyframe): one set of launches per frame -- two for passes of a few thousand seeds,
 * six beyond (svo_hip_df_set_small_pass_limit) -- instead of one set per keyframe.  The arguments of every batch are
 * checked before anything is enqueued.  Up to 8 batches go down per set of launches: with at most 8 the call updates all
 * batches or none; with more, a device failure in a later set (out of memory for its work area, a launch error) returns
 * the error while the earlier sets are already enqueued -- svo_hip_seed_batch_pending tells which batches then have a
 * pass to collect (DeviceSeedMirror collects exactly those). */
int svo_hip_seed_batch_update_group_async(int n_batches, svo_hip_seed_batch* const* batches, const svo_hip_pyramid* ref,
                                          const int* ref_slots, const svo_hip_pyramid* cur, int cur_slot,
                                          const svo_hip_camera* cam, const double* T_ref_w /* [n_batches][7] */,
                                          const double T_cur_w[7], const svo_hip_df_params* prm, int report_updated);
/* The pass of SEVERAL cameras -- each with its own current frame (slot cur_slot of `cur`), pose, keyframe flag and batches --
 * as ONE set of launches whatever the number of cameras and batches: the depth filter's counterpart of a tracker group.  This
 * form takes one `cam` that every camera shares; svo_hip_seed_batch_update_rig_async below takes a model per camera, and this
 * call is that one with `cam` repeated.  Camera c's batch k runs against keyframe slot ref_slots[k] of `ref` with pose T_ref_w[7 * k ..]
 * and against the camera's own current image, pose and report_updated.  Results per batch are bit-identical to one
 * svo_hip_seed_batch_update_group_async per camera; collect, pending, erase, download and mark_updated work on the batches
 * afterwards as after that call.  The form is chosen as there (two launches up to the small-pass limit, six beyond).
 * The table of the jobs (a batch's arrays, transforms, current slot, keyframe flag and camera), the map from every 256-seed block
 * to its job and the camera models of the pass live in device memory of the context: one packed transfer per call out of page-locked staging, both grow-only
 * (no allocator call after a warm-up call).  A call may follow another for other batches without a collect in between: the
 * staging area is rewritten only once the previous call's transfer has left it.
 * At most SVO_HIP_DF_CAMERAS_MAX_JOBS batches and SVO_HIP_DF_CAMERAS_MAX_RECORDS seed records (every batch rounded up to 256)
 * per call.  Everything is checked before anything is enqueued and a refused call changes nothing: SVO_HIP_ERR_INVALID for a
 * null argument, a batch of another context, a batch named twice (also under two cameras), a slot out of range, image sizes
 * that differ from `cam` and a capacity exceeded; SVO_HIP_ERR_STATE for a batch whose previous pass is not collected.  A call
 * without any batch returns SVO_HIP_OK and launches nothing.  A device failure after the first enqueue synchronises the stream
 * before it returns (nothing of the call is still in flight when the caller unwinds). */
#define SVO_HIP_DF_CAMERAS_MAX_JOBS 1024
#define SVO_HIP_DF_CAMERAS_MAX_RECORDS (1 << 20)
typedef struct {
  int n_batches;                          /* 0: the camera sits this pass out */
  svo_hip_seed_batch* const* batches;     /* [n_batches], all of the call's context */
  const int* ref_slots;                   /* [n_batches] slots of `ref` */
  const double* T_ref_w;                  /* [n_batches][7] */
  int cur_slot;                           /* slot of `cur` holding this camera's current frame */
  double T_cur_w[7];
  int report_updated;                     /* this camera's frame is a keyframe */
} svo_hip_seed_camera_pass;
int svo_hip_seed_batch_update_cameras_async(svo_hip_ctx* ctx, int n_cameras, const svo_hip_seed_camera_pass* passes,
                                            const svo_hip_pyramid* ref, const svo_hip_pyramid* cur,
                                            const svo_hip_camera* cam, const svo_hip_df_params* prm);
/* The same pass for a camera RIG: cams[c] is the model of passes[c]'s camera -- its own fx, fy, cx, cy and distortion.  The image
 * SIZE is common: the pyramids are shared, so every cams[c] must have the width and height of cams[0] and of `ref` and `cur`
 * (SVO_HIP_ERR_INVALID otherwise, also for a camera that sits the pass out, and for a null `cams`; checked with everything else
 * before anything is enqueued).  Every batch's results are bit-identical to svo_hip_seed_batch_update_group_async for its
 * camera alone with that camera's model; n equal models give what svo_hip_seed_batch_update_cameras_async gives.  The models
 * (with the pixel error angle 2 atan(1 / (2 |fx|)) each implies) travel behind the job table in the same packed transfer. */
int svo_hip_seed_batch_update_rig_async(svo_hip_ctx* ctx, int n_cameras, const svo_hip_seed_camera_pass* passes,
                                        const svo_hip_pyramid* ref, const svo_hip_pyramid* cur,
                                        const svo_hip_camera* cams /* [n_cameras] */, const svo_hip_df_params* prm);
/* diagnostic / tuning: passes of at most max_seeds seed records (sum over the batches of a call, each rounded up to 256)
 * run as TWO launches -- one wave takes its four seeds through geometry, search, alignment and update, then one workgroup
 * per batch writes the events -- instead of six; results are bit-identical.  0 switches the form off; at most 16384;
 * the default is 8192 (DESIGN.md section 8 has the crossover measurement). */
int svo_hip_df_set_small_pass_limit(svo_hip_ctx* ctx, int max_seeds);
/* 1 while a pass of the batch is enqueued and not collected yet, else 0 (also for NULL) */
int svo_hip_seed_batch_pending(const svo_hip_seed_batch* batch);
/* wait for the pass; *events points into page-locked memory owned by the batch (valid until its next update_async);
 * status_counts[7]: seeds per outcome of this pass, slot = status + 1 (slot 0 = SVO_HIP_SEED_ERASED ... slot 6 =
 * SVO_HIP_SEED_NAN).  Either output may be NULL. */
int svo_hip_seed_batch_collect(svo_hip_seed_batch* batch, const svo_hip_seed_event** events, int* n_events,
                               int32_t status_counts[7]);
int svo_hip_seed_batch_erase(svo_hip_seed_batch* batch, int n, const int32_t* indices);      /* host array */
/* state of every seed of the batch, erased ones included (alive[i] = 0); any output may be NULL; synchronises */
int svo_hip_seed_batch_download(svo_hip_seed_batch* batch, float* a, float* b, float* mu, float* sigma2, uint8_t* alive);
/* the batch's device arrays (tests, benchmarks): a, b, mu, sigma2 [n] f32, status [n] i32 of the last pass */
int svo_hip_seed_batch_arrays(svo_hip_seed_batch* batch, float** a_dev, float** b_dev, float** mu_dev, float** sigma2_dev,
                              int32_t** status_dev);

/* host-buffer convenience form of the above (copies in, runs, copies out, synchronises) */
int svo_hip_depth_filter_update(svo_hip_ctx* ctx, const svo_hip_pyramid* ref, int ref_slot,
                                const svo_hip_pyramid* cur, int cur_slot, const svo_hip_camera* cam,
                                const double T_ref_w[7], const double T_cur_w[7], int n, const double* px,
                                const double* f, const int32_t* level, float* a, float* b, float* mu,
                                const float* z_range, float* sigma2, const svo_hip_df_params* prm,
                                int32_t* status, double* z, double* xyz_world, int32_t* n_zmssd,
                                int32_t* n_align_iters, double* px_cur, int32_t* search_level);

/* ---- next rows: the two small Gauss-Newton refinements of FrameHandlerMono::processFrame ------
 * pose_optimizer::optimizeGaussNewton (I/pose_optimizer.h:36-45, pose_optimizer.cpp:31-181; caller
 * frame_handler_mono.cpp:226-229): motion-only refinement of frame->T_f_w_ over the features that have a point:
 * MAD scale, <= n_iter Tukey-weighted Gauss-Newton steps on the unit plane, covariance, outlier test.
 * Per frame b of the batch: n_feat[b] observations at [b][0..max_n): f[3] unit bearing (Feature::f), pos[3]
 * (Point::pos_), level (Feature::level), has_point u8 in/out (cleared where the reference sets
 * (*it)->point = NULL, pose_optimizer.cpp:154-157).  error_multiplier2 = cam->errorMultiplier2(). */
typedef struct {
  int32_t ran;             /* 0: no observation had a point -- the reference returns before touching anything */
  int32_t n_iter_done;     /* linear systems built and solved */
  int32_t n_deleted;       /* observations removed by the final test */
  int32_t pad_;
  uint64_t num_obs;        /* observations left (the reference's num_obs) */
  double T_f_w[7];         /* refined pose (rolled back when the last step was rejected) */
  double estimated_scale;  /* as returned through the reference's parameter (MAD scale * errorMultiplier2) */
  double error_init, error_final;
  double Cov[36];          /* frame->Cov_ */
} svo_hip_pose_opt_result;

int svo_hip_pose_optimize_batch_dev(svo_hip_ctx* ctx, int batch, int max_n, const int32_t* n_feat_dev,
                                    const double* T_f_w_dev, const double* f_dev, const double* pos_dev,
                                    const int32_t* level_dev, uint8_t* has_point_dev, double error_multiplier2,
                                    double reproj_thresh, int n_iter, svo_hip_pose_opt_result* results_dev);
/* host-buffer convenience form for one frame (copies in, runs, copies out, synchronises) */
int svo_hip_pose_optimize(svo_hip_ctx* ctx, int n, const double T_f_w[7], const double* f, const double* pos,
                          const int32_t* level, uint8_t* has_point, double error_multiplier2, double reproj_thresh,
                          int n_iter, svo_hip_pose_opt_result* result);

/* Point::optimize (I/point.h:74, point.cpp:130-192; caller FrameHandlerBase::optimizeStructure,
 * frame_handler_base.cpp:190-210) for n_points map points: pos[n][3] in/out; the observations of point p are
 * obs[obs_offset[p] .. obs_offset[p+1]) in the order of Point::obs_: pose of the observing frame (T_f_w[7]) and
 * the feature's bearing f[3].  iters (optional): linear systems solved per point. */
int svo_hip_point_optimize_batch_dev(svo_hip_ctx* ctx, int n_points, int n_iter, double* pos_dev,
                                     const int32_t* obs_offset_dev, const double* obs_T_f_w_dev,
                                     const double* obs_f_dev, int32_t* iters_dev);

/* host-buffer convenience form (copies in, runs, copies out, synchronises) */
int svo_hip_point_optimize_batch(svo_hip_ctx* ctx, int n_points, int n_iter, double* pos, const int32_t* obs_offset,
                                 const double* obs_T_f_w, const double* obs_f, int32_t* iters);

/* ---- one tracked frame on one stream: FrameHandlerMono::processFrame up to the pose refinement ------------------
 *      (frame_handler_mono.cpp:171-229; SURVEY 8f-1 / f-2 / f-4 chained behind a-1)
 *   new_frame->T_f_w_ = last_frame->T_f_w_ (:175) -> SparseImgAlign(kltMaxLevel, kltMinLevel, 30).run(last, new) (:186-188)
 *   -> Reprojector::reprojectMap(new_frame, overlap_kfs) (:203; reprojector.cpp:72-259 with Map::getCloseKeyframes,
 *   Point::getCloseViewObs, Matcher::findMatchDirect) -> pose_optimizer::optimizeGaussNewton (:226-229) -> last_frame_ =
 *   new_frame_ (:91), enqueued as one chain of kernels with ONE synchronisation at the end: the pose SparseImgAlign leaves is
 *   read by the later stages on the device, the frame's matches become the next call's reference features without
 *   leaving it, and only level 0 of the new image crosses the link (from page-locked staging).
 * The map the reprojector walks is a set of index tables uploaded when the map changes (svo_hip_tracker_set_map);
 * keyframe pyramids live in a batch owned by the tracker.  The counters the reprojector keeps on the points are advanced
 * on the device and returned with every frame; when it DELETES a point (reprojector.cpp:126-133,202-209) the pointer
 * graph changes (Map::safeDeletePoint, S/map.cpp:78-88: every observation lets go of the point, a keyframe that loses a key
 * feature chooses its key features again, Frame::removeKeyPoint): the device tables follow -- the point is unlinked there and
 * the affected keyframes re-select before the next frame with the reference's rule -- and the result says map_changed so that
 * the host applies the same deletions to its own objects; a new upload of the map is NOT needed for that.
 * Host code keeps the Map / Point / Feature objects and acts on the decisions.  The structure step, the scene depth, needNewKf
 * and Map::getFurthestKeyframe -- keyframe selection -- are one device call (svo_hip_tracker_finish_frame below), so the host
 * needs no poses or point positions of its own between two keyframes.  Relocalisation is a device job like everything
 * else between two keyframes (svo_hip_tracker_relocalize below); svo_hip_tracker_set_last_frame remains the way in for a last
 * frame the device's map does not hold (after initialisation). */
typedef struct svo_hip_tracker svo_hip_tracker;

typedef struct {
  /* capacities */
  int max_keyframes, max_points, max_obs, max_kf_features, max_candidates;
  int max_items;               /* candidates over all grid cells of one frame */
  int max_frame_features;      /* features of one frame (<= 2816) */
  int n_levels;                /* pyramid levels of a frame: max(Config::nPyrLevels(), Config::kltMaxLevel() + 1) (frame.cpp:63) */
  /* the values processFrame reads from svo::Config / the objects' Options */
  int klt_max_level, klt_min_level, sia_n_iter;    /* config.cpp:62-63; frame_handler_mono.cpp:186-187 */
  double sia_eps;                                  /* sparse_img_align.cpp:40 */
  int grid_size, max_fts, quality_min_fts;         /* Config::gridSize(), maxFts(), qualityMinFts() */
  int reproj_max_n_kfs;                            /* Reprojector::Options::max_n_kfs (<= 16) */
  int n_pyr_levels, align_max_iter;                /* Config::nPyrLevels(), Matcher::Options::align_max_iter */
  double pose_optim_thresh;                        /* Config::poseOptimThresh() */
  int pose_optim_num_iter;                         /* Config::poseOptimNumIter() */
} svo_hip_tracker_config;

/* the reference's defaults (config.cpp:56-84) and roomy capacities */
int svo_hip_tracker_default_config(svo_hip_tracker_config* cfg);

/* svo::Map as index tables (host arrays, copied in).  Keyframes in Map::keyframes_ order; kf_slot[k] = slot of keyframe
 * k's pyramid in the tracker's keyframe batch; kf_key_point[k][5] = point index of Frame::key_pts_[j]->point or -1;
 * kf_ftr_point = the point of every keyframe feature that has one, keyframe by keyframe in fts_ order
 * ([kf_ftr_offset[k], kf_ftr_offset[k+1])).  Points: Point::pos_, type_ (0 deleted, 1 candidate, 2 unknown, 3 good),
 * n_failed_reproj_, n_succeeded_reproj_, and their observations in Point::obs_ order ([pt_obs_offset[p],
 * pt_obs_offset[p+1])): keyframe INDEX the feature lies in, Feature::px / f / level, EDGELET flag and grad (both may be
 * NULL: corners).  cand_point: the points of MapPointCandidates::candidates_ in list order (their single observation is
 * the seed's feature). */
typedef struct {
  int n_kf;
  const int32_t* kf_slot;
  const double* T_kf_w;
  const int32_t* kf_key_point;
  const int32_t* kf_ftr_offset;
  const int32_t* kf_ftr_point;
  int n_points;
  const double* pt_pos;
  const int32_t* pt_type;
  const int32_t* pt_n_failed;
  const int32_t* pt_n_succeeded;
  const int32_t* pt_obs_offset;
  const int32_t* obs_kf;
  const double* obs_px;
  const double* obs_f;
  const int32_t* obs_level;
  const uint8_t* obs_edgelet;
  const double* obs_grad;
  int n_candidates;
  const int32_t* cand_point;
} svo_hip_tracker_map;

typedef struct {
  double T_f_w[7];              /* new_frame_->T_f_w_ as processFrame leaves it for last_frame_: the refined pose; the LAST
                                   frame's pose when the reprojector matched fewer than quality_min_fts points (:208-215) */
  double T_f_w_sia[7];          /* ... after SparseImgAlign::run (:188) */
  uint64_t sia_n_tracked;       /* img_align_n_tracked */
  int32_t sia_iters[SVO_HIP_MAX_LEVELS];
  int32_t sia_stop;
  int32_t n_features;           /* new_frame_->fts_.size(): features the reprojector added, in creation order */
  uint64_t n_matches, n_trials; /* reprojector_.n_matches_, n_trials_ */
  int32_t n_overlap;            /* overlap_kfs_.size() */
  int32_t map_changed;          /* 1: a point or candidate was deleted (its type is TYPE_DELETED in pt_type): apply Map::safeDeletePoint /
                                   deleteCandidatePoint to the host's objects; the device tables have followed already */
  int32_t overlap_kf[16];       /* overlap_kfs_[i].first as keyframe index */
  int32_t overlap_count[16];    /* overlap_kfs_[i].second */
  int32_t n_candidates;         /* candidates in all cells */
  int32_t items_overflow;       /* 1: more than max_items candidates (the excess was dropped: raise max_items) */
  svo_hip_pose_opt_result pose; /* sfba_*: ran == 0 when the refinement was not reached */
} svo_hip_track_result;

int svo_hip_tracker_create(svo_hip_ctx* ctx, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, svo_hip_tracker** out);
int svo_hip_tracker_destroy(svo_hip_tracker* trk);
/* grid geometry (Reprojector::initializeGrid, reprojector.cpp:44-55) and the keyframe pyramid batch (borrowed) */
int svo_hip_tracker_info(const svo_hip_tracker* trk, int* n_cells, int* grid_cols, int* grid_rows, svo_hip_pyramid** keyframe_pyramids);
/* The pyramid batch that holds the last frames of the tracker's group, and this camera's slot in it (0 for a lone tracker).
 * The batch is BORROWED: it is valid until the next call that tracks, relocalises or sets a last frame on this tracker or its
 * group (the two frame batches swap roles every tracked frame).  A pass that reads it (svo_hip_seed_batch_update_cameras_async)
 * must run on the tracker's context: the stream then orders the pass behind the track call and in front of the next one.
 * With svo_hip_tracker_info's keyframe batch (camera c's keyframe slot s is slot c * max_keyframes + s) a group's depth pass
 * needs no image upload and no pyramid build of its own.  SVO_HIP_ERR_STATE when the tracker has no last frame. */
int svo_hip_tracker_last_frame_pyramid(svo_hip_tracker* trk, const svo_hip_pyramid** pyr, int* slot);
/* keyframe images: level 0 from the host (pyramid built on the device), or the pyramid of the last tracked frame
 * (FrameHandlerMono: new_frame_->setKeyframe(); map_.addKeyframe(new_frame_), :284-330) */
int svo_hip_tracker_upload_keyframe(svo_hip_tracker* trk, int slot, const uint8_t* level0);
int svo_hip_tracker_keyframe_from_last_frame(svo_hip_tracker* trk, int slot);
/* The map as index tables (every index is checked here, on the host).  The last frame's features refer to map points by index: a
 * map with the same point numbering may be set between two tracked frames; if the new map has fewer points than the largest
 * index the last frame uses, the last frame is forgotten and svo_hip_tracker_set_last_frame has to follow.  A map that is
 * refused (an index out of range, a table above its capacity) changes nothing. */
int svo_hip_tracker_set_map(svo_hip_tracker* trk, const svo_hip_tracker_map* map);
/* the keyframes' key points as the device holds them ([n_kf][5] point indices, -1 = none): what was uploaded, advanced by the
 * re-selections that followed deletions (parity tests) */
int svo_hip_tracker_download_key_points(svo_hip_tracker* trk, int32_t* kf_key_point);
/* Point::pos_ of n points after FrameHandlerBase::optimizeStructure (frame_handler_base.cpp:190-210) */
int svo_hip_tracker_update_point_positions(svo_hip_tracker* trk, int n, const int32_t* point, const double* pos);
/* FrameHandlerBase::optimizeStructure (frame_handler_base.cpp:190-210) without the observations leaving the device: the host
 * selects the points as the reference does (std::nth_element by Point::last_structure_optim_) and passes their indices
 * (n <= 64, no duplicates); Point::optimize(n_iter) runs on each over the observations the map tables hold (keyframe pose +
 * bearing in Point::obs_ order), and the new positions go into the device's point table, into the solver's copy of the last
 * frame's points and to pos_out[n][3] (iters_out[n]: iterations taken, may be NULL).  One launch, one synchronisation;
 * replaces svo_hip_point_optimize_batch + svo_hip_tracker_update_point_positions between two tracked frames. */
int svo_hip_tracker_optimize_structure(svo_hip_tracker* trk, int n, const int32_t* point, int n_iter, double* pos_out, int32_t* iters_out);
/* last_frame_ from the host (after initialisation / relocalisation): its image (level0, or NULL = the keyframe pyramid in
 * kf_slot), pose and features: px[n][2], f[n][3], point[n] (index or -1) */
int svo_hip_tracker_set_last_frame(svo_hip_tracker* trk, const uint8_t* level0, int kf_slot, const double T_f_w[7], int n,
                                   const double* px, const double* f, const int32_t* point);
/* The tracker's own image buffer: width x height bytes of page-locked, device-mapped host memory the first kernel of a
 * frame reads level 0 from.  svo_hip_tracker_track copies the caller's image there; a caller whose camera frames can land
 * in this buffer (a cv::Mat header over it, Frame::img_pyr_[0] of the new frame) passes the buffer itself as level0 and
 * saves that copy (about 10 us of a 640x480 frame).  The buffer belongs to the tracker, is free again when
 * svo_hip_tracker_track returns, and lives until svo_hip_tracker_destroy. */
int svo_hip_tracker_image_buffer(svo_hip_tracker* trk, uint8_t** buffer);
/* An option of the SparseImgAlign solver this tracker uses.  SVO_HIP_SIA_OPT_REDUCTION only (see svo_hip_sia_set_option;
 * any other option: SVO_HIP_ERR_INVALID -- the chain fixes the solver's method, cost and arithmetic).  The cameras of a group
 * share one solver: set on a handle from svo_hip_tracker_group_camera it holds for EVERY camera of that group.  Takes
 * effect from the next tracked frame. */
int svo_hip_tracker_set_sia_option(svo_hip_tracker* trk, int option, int value);
/* One frame.  Outputs (host, any may be NULL except result): the new frame's features in creation order -- px[n][2],
 * f[n][3], level[n], point[n] (-1 where the pose refinement dropped the observation, pose_optimizer.cpp:154-157),
 * edgelet[n], grad[n][2], capacity max_frame_features -- and the point counters after the frame (capacity n_points of
 * the map).  The counter outputs cover the points the map had WHEN THE FRAME WAS TRACKED: svo_hip_tracker_last_result after
 * svo_hip_tracker_add_candidates still returns that many.  Synchronises once. */
int svo_hip_tracker_track(svo_hip_tracker* trk, const uint8_t* level0, svo_hip_track_result* result, double* feat_px,
                          double* feat_f, int32_t* feat_level, int32_t* feat_point, uint8_t* feat_edgelet, double* feat_grad,
                          int32_t* pt_type, int32_t* pt_n_failed, int32_t* pt_n_succeeded);

/* ---- several cameras: FrameHandlerMono::processFrame (frame_handler_mono.cpp:171-229) of N independent cameras per call.
 * north_star's "concurrent frame pairs" for the whole per-frame chain: N svo::FrameHandlerMono objects (N cameras, or N
 * sequences replayed side by side) each track one frame at a time; with N trackers on N host threads the HIP runtime's launch
 * path serialises them (measured: 5.5 k frames/s for one camera, 20 k for 4, 21-26 k for 8-16, whatever the number of hardware
 * queues: profiles/r05_cameras_threads.txt).  A group creates N trackers with one image size and one configuration that
 * share the SparseImgAlign solver (camera c = slot c), the frame and keyframe pyramid batches and the per-camera arrays of
 * the batched stages, and tracks one frame of EVERY camera with ONE chain of launches: every kernel of the chain takes one
 * workgroup (or one slice of its grid) per camera, the cameras' arguments come from a table in device memory.
 * A camera's handle (svo_hip_tracker_group_camera) takes every svo_hip_tracker_* call except _track and _destroy: its map,
 * its last frame, its keyframe slots (0 .. max_keyframes - 1, its own), structure optimisation, image buffer.  Outcomes are
 * bit for bit those of the same camera tracked by a lone svo_hip_tracker (tests/test_gpu_tracker_group.py) in one of two
 * ways.  By default (SVO_HIP_SIA_REDUCTION_PER_WAVE) only while the SparseImgAlign kernel shape is the same: it is chosen
 * by the largest feature count among the cameras' last frames and by the number of cameras (svo_hip_sia_last_run_mode), and a
 * camera that tracks beside a larger one gets the last bits of its SparseImgAlign pose from another grouping of the sums
 * than alone (rounding level on that frame; every later frame starts from that pose).  With
 * svo_hip_tracker_set_sia_option(SVO_HIP_SIA_OPT_REDUCTION, SVO_HIP_SIA_REDUCTION_TILE_ORDER) on the group AND on the lone
 * tracker nothing depends on the company: every camera equals its lone tracker whatever the other cameras hold
 * (tests/test_gpu_tracker_invariance.py).  cfg->max_items must be a multiple of 16 when n_cameras > 1.
 * The cameras of a RIG each have their own model: svo_hip_tracker_group_create_rig takes cams[n_cameras], cams[c] camera c's
 * fx, fy, cx, cy and distortion, and every stage of the chain, the per-handle calls (relocalisation, map edits,
 * svo_hip_tracker_mark_last_frame, the structure step) and the pose refinement's error multiplier |fx| use camera c's own:
 * camera c equals a lone svo_hip_tracker created with cams[c] (tests/test_gpu_tracker_rig.py).  The image SIZE is common -- the
 * pyramid batches, the grid and the page-locked image blocks are shared and sized once: SVO_HIP_ERR_INVALID for a camera whose
 * width or height differs from cams[0], for a null `cams`, n_cameras < 1 and for what svo_hip_tracker_create refuses, for any
 * camera; a refused call has allocated nothing.  svo_hip_tracker_group_create is the rig call with `cam` repeated. */
typedef struct svo_hip_tracker_group svo_hip_tracker_group;
int svo_hip_tracker_group_create(svo_hip_ctx* ctx, const svo_hip_camera* cam, const svo_hip_tracker_config* cfg, int n_cameras,
                                 svo_hip_tracker_group** out);
int svo_hip_tracker_group_create_rig(svo_hip_ctx* ctx, const svo_hip_camera* cams /* [n_cameras] */, const svo_hip_tracker_config* cfg,
                                     int n_cameras, svo_hip_tracker_group** out);
int svo_hip_tracker_group_destroy(svo_hip_tracker_group* group);
int svo_hip_tracker_group_camera(svo_hip_tracker_group* group, int index, svo_hip_tracker** camera);
/* One frame of every camera: level0[c] = camera c's new image (its svo_hip_tracker_image_buffer: no copy); results[n_cameras]
 * (may be NULL).  Synchronises once, for all cameras.  The cameras' features and point counters are read afterwards with
 * svo_hip_tracker_last_result on the handles that need them. */
int svo_hip_tracker_group_track(svo_hip_tracker_group* group, const uint8_t* const* level0, svo_hip_track_result* results);
/* One frame of SOME cameras: camera[n_active] names them (strictly increasing), level0[j] is camera[j]'s new image (its
 * svo_hip_tracker_image_buffer: no copy), results[n_active] (may be NULL) camera[j]'s result.  The cameras named are tracked
 * exactly as svo_hip_tracker_group_track tracks them -- one chain of launches whatever n_active, one synchronisation, features
 * read afterwards with svo_hip_tracker_last_result -- and every stage is launched n_active cameras wide: a group of 64 with one
 * camera in the call builds one pyramid, not 64.  n_active == n_cameras (the list is the identity then) makes the launches of
 * svo_hip_tracker_group_track and gives its bytes; svo_hip_tracker_group_track itself keeps refusing a null image.
 * A camera that SITS OUT is not touched: its map tables, key points and a pending key-point re-selection (it stays owed), its
 * last frame's features and pose, the solver slot prepared for its next frame, its result block (svo_hip_tracker_last_result
 * keeps returning it), the scratch the keyframe decision reads (svo_hip_tracker_finish_frame gives the decision it gave before)
 * and the bytes of its last frame's pyramid all stay as they were.  Only the cameras named need a map and a last frame: a
 * camera that was never set up may sit out.
 * The two frame batches: when at least half of the cameras are named they swap roles as in every tracked frame and the
 * pyramids of the cameras that sit out are copied into the new "last" batch; otherwise the batches keep their roles and the
 * new pyramids of the cameras named are copied back into it -- one launch either way, the smaller side moves.  So
 * svo_hip_tracker_last_frame_pyramid may return either batch after this call, for every camera the same one and with the bytes
 * of that camera's last frame in its slot: the batch stays BORROWED under the rule stated there (this call is one that tracks).
 * Outcomes are those of a lone svo_hip_tracker on the same frames in the two ways described above: unconditionally with
 * SVO_HIP_SIA_REDUCTION_TILE_ORDER on both sides; by default while the SparseImgAlign kernel shape is the same, which the cameras
 * NAMED choose -- their number and the largest feature count among their last frames.
 * n_active == 0: SVO_HIP_OK, nothing enqueued.  Refused before anything is enqueued or changed: SVO_HIP_ERR_INVALID for a null
 * group, n_active outside [0, n_cameras], a null `camera` or `level0` with n_active > 0, an index out of range, a list that is not
 * strictly increasing, a null image; SVO_HIP_ERR_STATE when a camera named lacks its map or its last frame.  A failure behind the
 * first enqueue synchronises the stream and has the solver slots of the cameras named gathered again by their next frame. */
int svo_hip_tracker_group_track_some(svo_hip_tracker_group* group, int n_active, const int32_t* camera /* [n_active] */,
                                     const uint8_t* const* level0 /* [n_active] */, svo_hip_track_result* results /* [n_active] */);
/* The outcome of the camera's last tracked frame again (same outputs as svo_hip_tracker_track; any may be NULL): a copy from
 * the camera's page-locked result block, no device call. */
int svo_hip_tracker_last_result(svo_hip_tracker* trk, svo_hip_track_result* result, double* feat_px, double* feat_f,
                                int32_t* feat_level, int32_t* feat_point, uint8_t* feat_edgelet, double* feat_grad,
                                int32_t* pt_type, int32_t* pt_n_failed, int32_t* pt_n_succeeded);

/* ---- the map grows in place (opt-in; svo_hip_tracker_set_map keeps working as before).  Two things change the map at frame
 * rate besides deletions and optimised positions: the depth filter converges seeds into point candidates, and the tracked
 * frame becomes a keyframe.  Both extend the device tables without the host flattening its pointer graph again.  Point,
 * keyframe and candidate indices that existed before keep their meaning, so the last frame stays valid across both calls.
 * Both take a lone tracker's handle or a handle from svo_hip_tracker_group_camera.  A keyframe leaves the map in place too
 * (svo_hip_tracker_remove_keyframe below).  None of the three renumbers POINTS: a deleted point keeps its index and its rows of
 * the pt_* tables, so n_points only grows with them; when svo_hip_tracker_add_candidates is refused for max_points,
 * svo_hip_tracker_compact_points (below) renumbers the living points in place and frees the room the dead ones held.  What
 * still needs svo_hip_tracker_set_map: anything that renumbers points or keyframes in another way than those two calls.
 *
 * svo_hip_tracker_add_candidates: what DepthFilter::updateSeeds (depth_filter.cpp:310-331) and
 * MapPointCandidates::newCandidatePoint (map.cpp:226-231) do for n converged seeds.  Host arrays: pos[n][3] the new points,
 * kf_index[n] the keyframe INDEX the seed's feature lies in (-1: that keyframe has left the map -- the point gets no
 * observation), px[n][2] / f[n][3] / level[n] / edgelet[n] (NULL: corners) / grad[n][2] (NULL: (1,0)) that feature.  The points
 * get the indices n_points .. n_points + n - 1 (*first_point = the first, may be NULL), Point::TYPE_CANDIDATE, both counters
 * 0; their observations go to the end of the observation tables and the points to the end of the candidate list, in argument
 * order.  Every index and capacity (max_points, max_obs, max_candidates, level < n_levels, kf_index < n_kf) is checked on the
 * host first: a refused call returns SVO_HIP_ERR_INVALID and changes nothing.  One packed transfer, one launch, no wait for
 * the device beyond the re-use of the staging area. */
int svo_hip_tracker_add_candidates(svo_hip_tracker* trk, int n, const double* pos, const int32_t* kf_index, const double* px,
                                   const double* f, const int32_t* level, const uint8_t* edgelet, const double* grad,
                                   int32_t* first_point);
/* svo_hip_tracker_promote_last_frame: the last TRACKED frame becomes keyframe *kf_index = n_kf with its pyramid in `slot`
 * (FrameHandlerMono::processFrame :267-276, map_.addKeyframe :312), from what the device holds of it:
 *   - pose = the frame's T_f_w; pyramid kept as svo_hip_tracker_keyframe_from_last_frame keeps it;
 *   - its features that still have a point form the keyframe's feature row in creation order, and each becomes an observation
 *     at the FRONT of its point's list (Point::addFrameRef, point.cpp:61-65) with the feature's px, f, level, edgelet flag, grad;
 *   - Frame::setKeyPoints (frame.cpp:84-146) over those features, from five empty slots;
 *   - MapPointCandidates::addCandidatePointToFrame (map.cpp:236-254): every candidate the frame observes becomes TYPE_UNKNOWN
 *     with n_failed_reproj_ = 0 and leaves the candidate list (compacted, order kept, entries that were -1 dropped); its seed
 *     feature joins the END of its own keyframe's feature row, in list order (none when its kf_index was -1);
 *     *n_promoted_candidates = how many.
 * A re-selection of key points the last frame's deletions still owe is applied first, on the rows as they were.  Checked
 * before anything is enqueued (SVO_HIP_ERR_INVALID, nothing changes): slot in range and held by no keyframe, n_kf <
 * max_keyframes, room in max_obs for the features with a point and in max_kf_features for them plus min(them, n_candidates)
 * seed features -- a worst-case bound, the real number is known only on the device.  SVO_HIP_ERR_STATE without a map or when
 * the last frame was not tracked (one from svo_hip_tracker_set_last_frame has no levels).  Synchronises once. */
int svo_hip_tracker_promote_last_frame(svo_hip_tracker* trk, int slot, int* kf_index, int* n_promoted_candidates);
/* svo_hip_tracker_remove_keyframe: keyframe kf_index leaves the device's map in place -- what Map::safeDeleteFrame
 * (map.cpp:41-64) does to the objects, with removePtFrameRef (:66-80), safeDeletePoint (:82-93), deletePoint (:95-99),
 * Point::deleteFrameRef (point.cpp:75-86) and MapPointCandidates::removeFrameCandidates / deleteCandidate (map.cpp:271-285,
 * :297-304).  FrameHandlerMono::processFrame (:303-308) makes this call after every new keyframe once the map holds
 * Config::maxNKfs() of them.  Takes a lone tracker's handle or a handle from svo_hip_tracker_group_camera.
 *   - A feature of the keyframe "has a point" when its point is not unlinked.  Such a point with at most two observations (all
 *     keyframes counted, this one included) is deleted: TYPE_DELETED, unlinked, no observations; *n_deleted_points = how
 *     many.  Any other loses its observation in the keyframe; the order of the rest, its counters and type stay.
 *   - A candidate whose seed feature (the last observation of its range) lies in the keyframe becomes TYPE_DELETED and
 *     unlinked and leaves the candidate list; *n_deleted_candidates = how many.  Candidates without an observation stay.
 *   - Row kf_index of kf_slot, T_kf_w, kf_key_point and of the feature rows disappears, later keyframes move down by one,
 *     every obs_kf above kf_index is decremented.  *slot_freed = the pyramid slot the keyframe held: free for the next
 *     promotion or upload.
 *   - The tables are left in the form a host flatten under the same point numbering writes: an unlinked point -- by this call
 *     or by an earlier frame -- has an empty observation range, is in no feature row and not in the candidate list (-1
 *     entries are dropped); row order and per-point observation order are kept.  n_ftr, n_obs and n_candidates of
 *     svo_hip_tracker_map_sizes are exact afterwards.
 *   - Key points: a re-selection the last frame's deletions still owe is applied first, on the rows as they were.  A keyframe
 *     that lost a key feature to a point deleted here chooses again before anything reads its key points, once, with
 *     Frame::removeKeyPoint's rule (the reference chooses again at every deletion: the outcomes differ only on exact ties
 *     of slot values); every other keyframe keeps its incumbents.
 *   - A feature of the device's last frame whose point was deleted here loses it (point -1; the solver skips it), as
 *     safeDeletePoint clears ftr->point of every observation.  The page-locked result block of the last tracked frame is not
 *     rewritten: svo_hip_tracker_last_result keeps returning the frame as it was tracked.
 * No table grows, so there is no capacity check.  Refused before anything is enqueued, nothing changes: SVO_HIP_ERR_STATE
 * without a map; SVO_HIP_ERR_INVALID for kf_index outside [0, n_kf) or a map of one keyframe (the reference removes only when
 * Config::maxNKfs() > 2).  Outputs may be NULL.  One launch, synchronises once. */
int svo_hip_tracker_remove_keyframe(svo_hip_tracker* trk, int kf_index, int* slot_freed, int* n_deleted_points,
                                    int* n_deleted_candidates);
/* svo_hip_tracker_compact_points: the dead points leave the device's tables in place and the living ones are renumbered.  Takes
 * a lone tracker's handle or a handle from svo_hip_tracker_group_camera.
 *   - A point is dead exactly when the device holds it as unlinked: deleted by a tracked frame (the reprojector's
 *     thresholds) or by svo_hip_tracker_remove_keyframe.  svo_hip_tracker_set_map unlinks nothing: a point uploaded as
 *     TYPE_DELETED is a living row until one of those deletes it.
 *   - Living points keep their relative order: the new index of a living point is the number of living points below it.
 *     old_to_new[n_points before the call] (may be NULL) receives that index, -1 for a dead point; *n_points_after (may be
 *     NULL) the number of living points.
 *   - A re-selection of key points the last frame's deletions still owe is applied first, on the rows as they were.
 *   - The tables end in the form a host flatten under the NEW numbering writes, the form the removal leaves: no row of a dead
 *     point in pt_pos, pt_type, pt_n_failed, pt_n_succeeded and pt_obs_offset, no observation of one, no feature-row entry
 *     and no candidate entry that points to one, -1 entries dropped; row order, per-point observation order and candidate
 *     order are kept.  svo_hip_tracker_map_sizes is exact afterwards, so the call also frees room in max_obs and
 *     max_kf_features.  Without a dead point every table keeps its bytes and old_to_new is the identity.
 *   - Every point index the device holds is rewritten: key points, feature rows, the candidate list and the features of the
 *     device's last frame (one whose point is dead gets -1 and the solver skips it; after a tracked frame there is none).
 *   - The page-locked result block of the last tracked frame is NOT rewritten: svo_hip_tracker_last_result keeps returning
 *     that frame as it was tracked, feat_point under the OLD numbering and the point counters for the OLD number of points.
 *     old_to_new is what translates it.  Results of frames tracked afterwards use the new numbering.
 * No table grows, so there is no capacity check; n_points == 0 is valid.  SVO_HIP_ERR_STATE without a map (nothing changes).
 * One launch, synchronises once. */
int svo_hip_tracker_compact_points(svo_hip_tracker* trk, int* n_points_after, int32_t* old_to_new);

/* ---- relocalisation against a keyframe of the device map: FrameHandlerMono::relocalizeFrame (frame_handler_mono.cpp:317-349)
 * without the host flattening its pointer graph: the keyframe's feature row, each point's observation in that keyframe, its pose
 * and pyramid slot, and the key points Map::getClosestKeyframe walks are all in the device tables.  The first two calls take a
 * lone tracker's handle or a handle from svo_hip_tracker_group_camera; each applies a re-selection of key points the last
 * frame's deletions still owe first, on the rows as they were, makes one small launch and synchronises once.
 *
 * svo_hip_tracker_closest_keyframe: Map::getClosestKeyframe (map.cpp:109-151) for a frame with pose T_f_w (NULL: the pose of the
 * device's last frame).  A keyframe is close when one of its five key points is Frame::isVisible from T_f_w (the first visible
 * one decides, as the reference's break); its distance is (T_f_w.translation_vec() - T_kf_w.translation_vec()).norm() -- the
 * translation of T_f_w, not pos(); squares summed in x, y, z order, uncontracted, then sqrt.  *kf_index = the close keyframe with
 * the smallest distance, the LOWER index on a tie (std::list::sort is stable over keyframes_ order); *distance its distance;
 * *n_close the close keyframes, counted before the exclusion (the last two may be NULL).  exclude_kf (-1: none) is the
 * reference's "close_kfs.front().first != frame" branch: the host knows whether its frame is a keyframe of the map and names
 * it; that keyframe is skipped.  When no candidate is left *kf_index = -1 and the call returns SVO_HIP_OK (the reference reads
 * front() of an empty list there: behaviour defined here).  SVO_HIP_ERR_STATE without a map, and for
 * T_f_w == NULL without a last frame. */
int svo_hip_tracker_closest_keyframe(svo_hip_tracker* trk, const double T_f_w[7], int exclude_kf, int* kf_index, int* n_close,
                                     double* distance);
/* svo_hip_tracker_last_frame_from_keyframe: last_frame_ = ref_keyframe (frame_handler_mono.cpp:337) from the device's own tables.
 *   - pose: row kf_index of T_kf_w; pyramid: the keyframe's slot, copied device to device into the last frame's pyramid (what
 *     svo_hip_tracker_set_last_frame(level0 = NULL, kf_slot) does);
 *   - features: the entries of the keyframe's feature row whose point is living (not unlinked), in row order = fts_ order, the
 *     order SparseImgAlign::precomputeReferencePatches walks.  Entries of unlinked points are DROPPED, not kept as point = -1; a
 *     point uploaded as TYPE_DELETED but never unlinked is a living row, as everywhere else;
 *   - px and f of a feature: the point's observation with obs_kf == kf_index -- the FIRST such observation in the point's
 *     observation order, should a keyframe observe a point twice.  (An entry whose point has no observation in the keyframe is no
 *     feature of it and is dropped too; tables a host flatten writes hold none.)
 * *n_features (may be NULL) = the features the last frame holds now.  Afterwards the tracker is exactly where
 * svo_hip_tracker_set_last_frame leaves it: the last frame is not a tracked one (svo_hip_tracker_promote_last_frame refuses it),
 * the solver's inputs are gathered again before the next frame, and the page-locked result block of the last tracked frame is
 * not rewritten.  Refused with nothing changed: SVO_HIP_ERR_STATE without a map; SVO_HIP_ERR_INVALID for kf_index outside
 * [0, n_kf), and when the living entries exceed max_frame_features (known only on the device: counted first, then decided).
 * A camera of a group relocalises with this call followed by svo_hip_tracker_group_track, without the gate. */
int svo_hip_tracker_last_frame_from_keyframe(svo_hip_tracker* trk, int kf_index, int* n_features);
/* svo_hip_tracker_relocalize: FrameHandlerMono::relocalizeFrame (:317-349) as one call, for a lone tracker.
 *   1. The reference keyframe is kf_index when kf_index >= 0, else svo_hip_tracker_closest_keyframe's answer for T_f_w_init
 *      (last_frame_->T_f_w_; NULL: the pose of the device's last frame) with exclude_kf applied.  When none is close:
 *      reloc->kf_index = -1, accepted = 0, SVO_HIP_OK, nothing changed -- the reference returns RESULT_FAILURE before it touches
 *      the new frame's pose; here the device's last frame is simply kept.
 *   2. The gate: the new image goes up and its pyramid is built as in svo_hip_tracker_track; the last frame becomes the keyframe
 *      as in svo_hip_tracker_last_frame_from_keyframe; SparseImgAlign(kltMaxLevel, kltMinLevel, sia_n_iter, GaussNewton)
 *      .run(ref_keyframe, new_frame) runs on the tracker's solver (its options, its SVO_HIP_SIA_OPT_REDUCTION) with T_ref_w = the
 *      keyframe's pose and T_cur_w_init = T_f_w_init (:329-333).
 *   3. gate_n_tracked > min_tracked (the reference's 30): accepted = 1 and the chain of svo_hip_tracker_track runs on the same
 *      image with last_frame_ = ref_keyframe; as in the reference it starts SparseImgAlign again from the keyframe's own pose
 *      (:175) -- the gate's pose is reported, not used.  result and the feature / counter outputs (those of
 *      svo_hip_tracker_track; any may be NULL) are that frame's, and the new frame is the device's last frame like any tracked
 *      one (svo_hip_tracker_promote_last_frame works on it).  Otherwise accepted = 0: the map tables and point counters are
 *      untouched (the gate only reads), the device's last frame is the new image with zero features and the pose T_f_w_gate --
 *      what addImage (:90) leaves in last_frame_, of which the reference's next attempt reads only that pose -- and result is
 *      not written.
 * Synchronises after the choice (the keyframe's feature count steers the solver's launch), after the gate and at the end of the
 * chain.  Refused before anything is enqueued, nothing changed: SVO_HIP_ERR_STATE without a map, for T_f_w_init == NULL
 * without a last frame, and for a handle of a group of more than one camera (a group tracks all its cameras per call);
 * SVO_HIP_ERR_INVALID for kf_index >= n_kf, min_tracked < 0, a NULL level0 / reloc.  SVO_HIP_ERR_INVALID with the last frame
 * kept when the keyframe's living features exceed max_frame_features.  On every error path after the first enqueue the stream
 * is synchronised before the call returns. */
typedef struct {
  int32_t kf_index;          /* the reference keyframe (the argument, or the device's choice); -1: none was close */
  int32_t n_close;           /* valid when the device chose */
  int32_t accepted;          /* 1: gate_n_tracked > min_tracked and the frame went through processFrame's stages */
  int32_t gate_stop;
  uint64_t gate_n_tracked;   /* img_align_n_tracked of :333 */
  int32_t gate_iters[SVO_HIP_MAX_LEVELS];
  double T_f_w_gate[7];      /* new_frame_->T_f_w_ as img_align.run leaves it (:333) */
} svo_hip_reloc_result;
int svo_hip_tracker_relocalize(svo_hip_tracker* trk, const uint8_t* level0, int kf_index, int exclude_kf, const double T_f_w_init[7],
                               int min_tracked, svo_hip_reloc_result* reloc, svo_hip_track_result* result, double* feat_px,
                               double* feat_f, int32_t* feat_level, int32_t* feat_point, uint8_t* feat_edgelet, double* feat_grad,
                               int32_t* pt_type, int32_t* pt_n_failed, int32_t* pt_n_succeeded);
/* ---- the structure step and the keyframe decision in one device call: what FrameHandlerMono::processFrame does behind the pose
 * refinement (frame_handler_mono.cpp:242-260, :305) from what the device holds already -- the last frame's pose and point
 * indices, the overlap keyframes the reprojector chose, the point positions and the keyframe poses.
 *
 * svo_hip_tracker_finish_frame, in ONE launch of one workgroup with one wait (the page-locked flag of
 * svo_hip_tracker_optimize_structure, the stream's synchronisation as the fall-back):
 *   1. optimizeStructure: exactly svo_hip_tracker_optimize_structure(n, point, n_iter, pos_out, iters_out) -- same checks, same
 *      outputs, same bits (one device function serves both kernels).  n == 0 skips the step.
 *   2. behind a barrier, on the positions just written:
 *      - frame_utils::getSceneDepth (frame.cpp:200-221): z = (T_f_w * pos_).z() of every feature of the device's last frame that
 *        has a point.  n_depths counts the depths that are numbers, n_nan_depths the NaNs (excluded).  depth_mean is
 *        vk::getMedian (math_utils.h:125-131): the element of rank floor(n_depths / 2) in ascending order, the exact order
 *        statistic (a radix select over order-preserving 64-bit keys, no sort, no float atomics); depth_min is fmin over the
 *        depths from DBL_MAX.  With n_nan_depths > 0 or without any depth depth_mean is NaN (the reference leaves it
 *        undefined in both cases: behaviour defined here).
 *      - needNewKf(depth_mean) (:391-403) over the overlap keyframes of the last tracked frame in overlap_kfs_ order:
 *        rel = T_f_w * kf->pos(); false at the first keyframe with fabs(rel.x)/depth_mean < d && fabs(rel.y)/depth_mean < d*0.8
 *        && fabs(rel.z)/depth_mean < d*1.3 (d = kf_select_min_dist = Config::kfSelectMinDist(), an argument because the
 *        configuration's size is fixed); blocking_kf names that keyframe.  A NaN depth_mean compares false: need_new_kf = 1.
 *      - Map::getFurthestKeyframe(frame->pos()) (map.cpp:156-169): dist = (kf->pos() - pos).norm(), squares summed in x, y, z
 *        order; dist > maxdist from 0.0, so the lowest index wins a tie, a NaN never wins and furthest_kf = -1 when every
 *        keyframe sits at the frame's position.
 * overlap_valid: the overlap keyframes are those of the last tracked frame and still name keyframes of the map.
 * svo_hip_tracker_track, svo_hip_tracker_group_track and an accepted svo_hip_tracker_relocalize set it;
 * svo_hip_tracker_set_map, _promote_last_frame, _remove_keyframe, _set_last_frame, _last_frame_from_keyframe and a refused
 * relocalisation gate clear it (each renumbers keyframes or replaces the frame); _optimize_structure,
 * _update_point_positions, _add_candidates and _compact_points keep it.  With the flag clear the call succeeds all the same:
 * depths and the furthest keyframe are valid for any last frame (processSecondFrame after svo_hip_tracker_set_last_frame),
 * need_new_kf = -1 and blocking_kf = -1.
 * Apart from the structure step's positions the call only reads: it applies no owed re-selection of key points (it reads no
 * key points) and leaves the page-locked result block of the last tracked frame alone.  Takes a lone tracker's handle or a
 * handle from svo_hip_tracker_group_camera.  Refused before anything is enqueued, nothing changed: SVO_HIP_ERR_INVALID for
 * what svo_hip_tracker_optimize_structure refuses, for decision == NULL and for a kf_select_min_dist that is NaN or negative;
 * SVO_HIP_ERR_STATE without a map or without a last frame. */
typedef struct {
  int32_t n_depths;          /* features of the device's last frame that have a point and whose depth is a number */
  int32_t n_nan_depths;      /* ... whose depth is NaN */
  double  depth_mean;        /* vk::getMedian: the element of rank floor(n_depths/2) in ascending order (the UPPER median for even n) */
  double  depth_min;         /* fmin over the depths, starting from DBL_MAX (NaNs skipped, as fmin skips them) */
  int32_t overlap_valid;     /* 1: the overlap keyframes of the last tracked frame still name keyframes of the map */
  int32_t need_new_kf;       /* needNewKf(depth_mean): 1 / 0; -1 when !overlap_valid */
  int32_t blocking_kf;       /* keyframe index of the FIRST overlap keyframe, in overlap_kfs_ order, that makes it return false; -1 */
  int32_t furthest_kf;       /* Map::getFurthestKeyframe(last frame's pos()): keyframe index, -1: none */
  double  furthest_distance; /* its distance, 0.0 without one */
  double  pos[3];            /* Frame::pos() of the last frame */
} svo_hip_kf_decision;
int svo_hip_tracker_finish_frame(svo_hip_tracker* trk, int n, const int32_t* point, int n_iter, double* pos_out, int32_t* iters_out,
                                 double kf_select_min_dist, svo_hip_kf_decision* decision);
/* The same for every camera of a group in ONE launch (workgroup c = camera c) with ONE wait.  req[c]: camera c's structure
 * request (req == NULL: n = 0 for all).  A camera without a map or without a last frame sits out: camera_ok[c] = 0, its
 * decision is zero-filled and its request has to be n == 0; the others get camera_ok[c] = 1 and, bit for bit, the positions and
 * the decision svo_hip_tracker_finish_frame gives on their handle.  Every request is checked before anything is enqueued: one
 * refused request (SVO_HIP_ERR_INVALID, as above) refuses the call for every camera and changes nothing. */
typedef struct { int32_t n; const int32_t* point; int32_t n_iter; double* pos_out; int32_t* iters_out; } svo_hip_structure_request;
int svo_hip_tracker_group_finish_frames(svo_hip_tracker_group* group, const svo_hip_structure_request* req /*[n_cameras], may be NULL: n = 0 for all*/,
                                        double kf_select_min_dist, svo_hip_kf_decision* decisions /*[n_cameras]*/, int32_t* camera_ok /*[n_cameras]*/);

/* diagnostics and parity tests: the sizes of the tables the device holds, and the tables themselves in svo_hip_tracker_map's
 * layout (the key points with the owed re-selections applied).  The caller's buffers hold at least the sizes
 * svo_hip_tracker_map_sizes reports (kf_ftr_offset n_kf + 1, pt_obs_offset n_points + 1); a NULL pointer skips its table.
 * n_kf / n_points / n_candidates are filled in.  svo_hip_tracker_download_map synchronises. */
typedef struct {
  int n_kf;
  int32_t* kf_slot;
  double* T_kf_w;
  int32_t* kf_key_point;
  int32_t* kf_ftr_offset;
  int32_t* kf_ftr_point;
  int n_points;
  double* pt_pos;
  int32_t* pt_type;
  int32_t* pt_n_failed;
  int32_t* pt_n_succeeded;
  int32_t* pt_obs_offset;
  int32_t* obs_kf;
  double* obs_px;
  double* obs_f;
  int32_t* obs_level;
  uint8_t* obs_edgelet;
  double* obs_grad;
  int n_candidates;
  int32_t* cand_point;
} svo_hip_tracker_map_out;
int svo_hip_tracker_map_sizes(const svo_hip_tracker* trk, int* n_kf, int* n_ftr, int* n_points, int* n_obs, int* n_candidates);
int svo_hip_tracker_download_map(svo_hip_tracker* trk, svo_hip_tracker_map_out* out);

/* The 6x6 pivoted LDL^T solve both Gauss-Newton solvers use (x = H.ldlt().solve(b), Eigen 3.4 semantics incl. the
 * pseudo-inverse of D), n systems from host buffers: exposed so that the parity tests can show it is bit-identical
 * to Eigen's result. */
int svo_hip_ldlt6_solve_batch(svo_hip_ctx* ctx, int n, const double* H /*[n][36]*/, const double* b /*[n][6]*/,
                              double* x /*[n][6]*/);

/* ---- next row: the producer of depth-filter seeds --------------------------------------------
 * FastDetector::detect (I/feature_detection.h:90-103, feature_detection.cpp:77-122; called by
 * DepthFilter::initializeSeeds, depth_filter.cpp:129-151): cv::FAST(img, kp, 10, true) on the first n_pyr_levels
 * levels of pyramid slot `slot`, one corner per grid cell (cell_size level-0 pixels) chosen by vk::shiTomasiScore,
 * strictly above detection_threshold; cells flagged in occupancy[grid_rows*grid_cols] (setExistingFeatures) are
 * skipped.  Outputs in cell order (capacity = number of cells): px[n][2] level-0 pixel, optional f[n][3] =
 * cam->cam2world(px) (distortion-free cameras only), level[n], optional score[n]; *n_out = n.
 * The final test is the reference's: the float score against the double detection_threshold.  Where the threshold's f32
 * rounding lies above it (10.1, not 10.0), every cell without a winner yields the reference's Feature(px (0,0), level 0),
 * with score (float)detection_threshold.  -0.0 counts as 0.0; NaN yields no feature.  A negative detection_threshold is
 * refused with SVO_HIP_ERR_INVALID by both entry points before anything is launched. */
int svo_hip_detect_grid(int width, int height, int cell_size, int* grid_cols, int* grid_rows);
int svo_hip_detect_features_dev(svo_hip_ctx* ctx, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera* cam,
                                int n_pyr_levels, int cell_size, const uint8_t* occupancy_dev,
                                double detection_threshold, int32_t* n_out_dev, double* px_dev, double* f_dev,
                                int32_t* level_dev, float* score_dev);
/* host-buffer convenience form (copies in, runs, copies out, synchronises) */
int svo_hip_detect_features(svo_hip_ctx* ctx, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera* cam,
                            int n_pyr_levels, int cell_size, const uint8_t* occupancy, double detection_threshold,
                            int32_t* n_out, double* px, double* f, int32_t* level, float* score);
/* Seed::Seed for n new seeds (depth_filter.cpp:36-45): a = b = 10, mu = 1/depth_mean, z_range = 1/depth_min,
 * sigma2 = z_range^2/36 */
int svo_hip_seed_init_batch_dev(svo_hip_ctx* ctx, int n, double depth_mean, double depth_min, float* a_dev, float* b_dev,
                                float* mu_dev, float* z_range_dev, float* sigma2_dev);

/* ---- a new keyframe's seeds, detected and created on the device ------------------------------------------------
 * What DepthFilter does when a keyframe is queued (depth_filter.cpp:191-229): updateSeeds(kf) marks the detector grid
 * with the px_cur of every seed it updated (:302-306), initializeSeeds(kf) (:129-151) marks the keyframe's own features
 * (setExistingFeatures, feature_detection.cpp:47-56), detects, creates one Seed per new feature (:36-45) and the
 * detector resets its grid (feature_detection.cpp:121).  Here the grid is a plain device buffer of grid_cols * grid_rows
 * bytes (svo_hip_detect_grid, svo_hip_malloc) -- what svo_hip_detect_features_dev reads as occupancy_dev -- and every
 * step marks, reads or clears it where it lies.
 *
 * Marking is AbstractDetector::setGridOccpuancy (feature_detection.cpp:58-64): cell
 *   k = (int)(px[1] / cell_size) * grid_cols + (int)(px[0] / cell_size),
 * a double divided by an int and truncated towards zero; the flat index is the only range test, as in the reference
 * (a pixel beyond the width whose k is valid marks the next row's cell).  Where the reference's .at() would throw or
 * its cast is undefined -- k outside [0, grid_cols * grid_rows), a non-finite coordinate, a quotient beyond int --
 * nothing is marked.  The only byte marking ever writes is 1. */

/* setExistingFeatures over n level-0 pixels px[n][2]: enqueued on the context stream, does not wait; n = 0 is a no-op */
int svo_hip_grid_mark_px_dev(svo_hip_ctx* ctx, int n, const double* px_dev, int cell_size, int grid_cols, int grid_rows,
                             uint8_t* occupancy_dev);
/* the same from a host array: the pixels are staged through the context's page-locked area (the call returns with that
 * one transfer in flight; the area's next user waits for it) and svo_hip_grid_mark_px_dev runs behind it */
int svo_hip_grid_mark_px(svo_hip_ctx* ctx, int n, const double* px_host, int cell_size, int grid_cols, int grid_rows,
                         uint8_t* occupancy_dev);
/* depth_filter.cpp:302-306 for a keyframe pass: the cell of px_cur of every seed whose status in the batch's last pass is
 * >= SVO_HIP_SEED_UPDATED (updated, converged, NaN) -- the seeds a report_updated = 1 pass reports, without the events.
 * The gate is the status, never px_cur: SVO_HIP_SEED_NO_MATCH seeds hold a non-finite px_cur, erased seeds a stale one.
 * Enqueued behind whatever the batches' stream holds: legal while the pass is pending and after its collect, until the
 * batch's next update.  One launch per set of up to 8 batches.  SVO_HIP_ERR_INVALID before anything is enqueued for
 * batches of different contexts, a NULL batch or grid, non-positive sizes. */
int svo_hip_seed_batch_mark_updated(int n_batches, svo_hip_seed_batch* const* batches, int cell_size, int grid_cols,
                                    int grid_rows, uint8_t* occupancy_dev);
/* setExistingFeatures(new_frame->fts_) from what the device holds: all features of the tracker's last frame, those
 * whose point the pose refinement dropped included (they stay in fts_, pose_optimizer.cpp:154-157).  A lone tracker's
 * or a group camera's handle; before or after svo_hip_tracker_promote_last_frame, after a removal or a compaction
 * (pixels do not move).  Reads tracker state only.  SVO_HIP_ERR_STATE without a last frame.  SYNCHRONISES the
 * tracker's stream before it returns, so that a grid owned by another context (the depth filter's) may be read or
 * marked there next. */
int svo_hip_tracker_mark_last_frame(svo_hip_tracker* trk, int cell_size, int grid_cols, int grid_rows,
                                    uint8_t* occupancy_dev);
/* initializeSeeds (depth_filter.cpp:129-151) as one device call: the detection of svo_hip_detect_features_dev -- same
 * kernels, same refusals, same threshold quirk, same rules for f (cam is required here: every seed has a bearing) --
 * written straight into a block of the context's seed-batch pool: px / f / level of the new features, the Seed
 * constructor's a, b, mu, z_range, sigma2 (:36-45, as svo_hip_seed_init_batch_dev), alive = 1, status =
 * SVO_HIP_SEED_ERASED until the first pass.  The block is laid out for the grid's cell count, the upper bound of n, and
 * is taken from the pool's capacity class of the CELL COUNT, not of n (n is not known when the block is taken).
 * occupancy_dev may be NULL (no cell is occupied); with clear_occupancy the grid is zeroed behind the detection
 * (resetGrid(), feature_detection.cpp:121).  One synchronisation.  *n = number of new seeds; the host outputs px[n][2],
 * f[n][3], level[n], score[n] (capacity: the cell count) may each be NULL.  n = 0 returns SVO_HIP_OK with *batch = NULL
 * and the block back in the pool; a refused call takes no block.  The batch is an ordinary svo_hip_seed_batch. */
int svo_hip_seed_batch_create_detected(svo_hip_ctx* ctx, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera* cam,
                                       int n_pyr_levels, int cell_size, uint8_t* occupancy_dev, int clear_occupancy,
                                       double detection_threshold, double depth_mean, double depth_min,
                                       svo_hip_seed_batch** batch, int32_t* n, double* px, double* f, int32_t* level,
                                       float* score);

/* ---- the bootstrap on the device: KLT tracking of the first frame's features ---------------------------------------
 * KltHomographyInit (I/initialization.h, S/initialization.cpp): addFirstFrame (:32-51) keeps the first frame's features,
 * addSecondFrame (:61-75) tracks them into every following frame with trackKlt (:180-226) -- cv::calcOpticalFlowPyrLK with a
 * 30 x 30 window, maxLevel 4, 30 iterations, eps 0.001, OPTFLOW_USE_INITIAL_FLOW -- erases the lost ones for good, forms the
 * bearings f_cur and the disparities, and returns NO_KEYFRAME until their median (vk::getMedian: the order statistic of rank
 * n / 2) reaches Config::initMinDisparity().  A handle holds that state for n_cameras cameras of one image size; any subset
 * of them is tracked by one call.  computeFundamental (:260-329) and the rest of addSecondFrame (:77-138) follow below
 * (svo_hip_klt_two_view); computeHomography (:232-258), the planar path the reference has switched off, is not built.
 *
 * OpenCV is not part of the reference's tree: PARITY UNPINNED.  The algorithm is written down in tests/klt_reference.py
 * (Gaussian pyramid by cv::pyrDown's integer arithmetic, levels while both sides exceed the window; Scharr derivatives;
 * 14-bit bilinear weights; the iteration and its exits) and the device computes that model's numbers bit for bit.  The
 * departures from OpenCV are listed in DESIGN.md section 7: the five window sums are exact integer sums converted to float
 * once; samples beyond the image are BORDER_REFLECT_101 values, derivatives beyond it are zero; the median of no disparity
 * is NaN. */
typedef struct svo_hip_klt svo_hip_klt;
typedef struct { int win_size, max_level, max_iter; double eps, min_eig_threshold; } svo_hip_klt_params;  /* 30, 4, 30, 1e-3, 1e-4 */
typedef struct { int n_in, n_tracked, n_levels; double disparity_median; } svo_hip_klt_result;
int svo_hip_klt_default_params(svo_hip_klt_params* params);                                     /* trackKlt's constants (:189-201) */
/* All device and page-locked memory of the handle is taken here: svo_hip_klt_track makes no allocator call.  params may be
 * NULL.  SVO_HIP_ERR_INVALID: win_size outside 3..30 (the window's template lives in LDS), an image not larger than the
 * window, n_cameras or max_features < 1. */
int svo_hip_klt_create(svo_hip_ctx* ctx, int width, int height, int n_cameras, int max_features, const svo_hip_klt_params* params,
                       svo_hip_klt** out);
int svo_hip_klt_destroy(svo_hip_klt* klt);
/* the Gaussian pyramid's shape: n_levels and the level sizes (arrays of SVO_HIP_MAX_LEVELS, each may be NULL) */
int svo_hip_klt_info(const svo_hip_klt* klt, int* n_levels, int* level_width, int* level_height);
/* addFirstFrame (:32-51) with the features from the host: px[n][2] as the reference's cv::Point2f, f[n][3]; the image is
 * level 0 of pyramid slot `slot` (copied: the caller's pyramid may change afterwards).  px_cur starts as px_ref (:49).
 * n = 0 is legal.  The `< 100 features` gate of :42 is the caller's.  Synchronises. */
int svo_hip_klt_set_reference(svo_hip_klt* klt, int camera, const svo_hip_pyramid* pyr, int slot, int n, const float* px, const double* f);
/* addFirstFrame as one call (detectFeatures, :154-174): svo_hip_detect_features_dev -- same kernels, refusals and threshold
 * quirk, no occupancy -- straight into the handle, px rounded to f32 as cv::Point2f(ftr->px[0], ftr->px[1]) rounds it.
 * *n = the number of features found.  If that exceeds max_features the call returns SVO_HIP_ERR_INVALID and the camera is
 * left without a reference (the count is known only after the detection).  Synchronises. */
int svo_hip_klt_set_reference_detected(svo_hip_klt* klt, int camera, const svo_hip_pyramid* pyr, int slot, const svo_hip_camera* cam,
                                       int n_pyr_levels, int cell_size, double detection_threshold, int32_t* n);
/* OPTFLOW_USE_INITIAL_FLOW with a motion prior (the remark at :196): px_cur[n][2] replaces the flow the next call starts
 * from; n must be the camera's current feature count. */
int svo_hip_klt_set_flow(svo_hip_klt* klt, int camera, int n, const float* px_cur);
/* trackKlt (:180-226) and the disparity median (:72) for the n listed cameras in one set of launches: camera cameras[i]
 * reads its current image from level 0 of slot slots[i] of `cur` (any pyramid batch of the context with the handle's image
 * size: a user's, or a tracker group's frame batch through svo_hip_tracker_last_frame_pyramid) and forms its bearings with
 * cams[i].  Lost features leave the camera's lists for good, px_cur is carried to the next call as its initial flow.  One
 * synchronisation.  n_tracked = 0 gives a NaN median.  Before anything is enqueued: SVO_HIP_ERR_INVALID for a camera out of
 * range or listed twice, a pyramid of another size or context, a slot out of range; SVO_HIP_ERR_STATE for a camera
 * without a reference. */
int svo_hip_klt_track(svo_hip_klt* klt, int n, const int* cameras, const svo_hip_pyramid* cur, const int* slots,
                      const svo_hip_camera* cams /*[n]*/, svo_hip_klt_result* results /*[n]*/);
/* the camera's lists as trackKlt leaves them (:203-225): px_ref[n][2], px_cur[n][2], f_ref[n][3], f_cur[n][3], disparity[n],
 * index[n] (each surviving feature's position in the set_reference order); each may be NULL.  f_cur and disparity are
 * defined after a svo_hip_klt_track.  Synchronises. */
int svo_hip_klt_download(svo_hip_klt* klt, int camera, int32_t* n, float* px_ref, float* px_cur, double* f_ref, double* f_cur,
                         double* disparity, int32_t* index);
/* a level of the camera's Gaussian pyramid (tests): the previous image's (current = 0, levels 0..) or the last tracked
 * image's (current = 1, levels 1..: its level 0 stays in the caller's pyramid) */
int svo_hip_klt_download_level(svo_hip_klt* klt, int camera, int current, int level, uint8_t* out);

/* ---- the bootstrap on the device: pose and first map points from the KLT lists -----------------------------------------
 * The rest of KltHomographyInit::addSecondFrame (S/initialization.cpp:77-138) on the lists a svo_hip_klt handle holds:
 * computeFundamental (:260-329) -- cv::findFundamentalMat(FM_RANSAC) and cv::recoverPose restated, then the reference's own
 * vk::computeInliers and Quaterniond(R) --, the init_min_inliers gate (:85), the scene-depth median over ALL xyz_in_cur and
 * the map scale (:92-105), the second frame's pose (:108-115), and for every inlier the gate of :123 and its position in the
 * world (:125).  The Point and Feature objects of :126-136 are the host's.
 *
 * OpenCV is not part of the reference's tree: PARITY UNPINNED.  The algorithm is written down in tests/two_view_reference.py
 * and the device computes that model's numbers bit for bit.  A fixed number of hypotheses replaces OpenCV's adaptive count;
 * hypothesis h samples 8 distinct correspondences as a function of (seed, h, draw, n) alone, solves the 8-point system on
 * Hartley-normalised coordinates by Gaussian elimination with complete pivoting, and is scored by the count of
 * correspondences whose larger squared epipolar distance is <= (reproj_thresh / errorMultiplier2)^2; the winner is the
 * highest count, the lowest index among equals.  Its four pose candidates are ranked by the number of masked
 * correspondences with both ray parameters of vk::triangulateFeatureNonLin positive.  DESIGN.md section 7 lists the
 * departures. */
enum {
  SVO_HIP_TWO_VIEW_OK = 0,            /* pose, scale and points are valid */
  SVO_HIP_TWO_VIEW_TOO_FEW = 1,       /* fewer than 8 correspondences */
  SVO_HIP_TWO_VIEW_NO_MODEL = 2,      /* every hypothesis degenerate */
  SVO_HIP_TWO_VIEW_CHEIRALITY = 3,    /* the gate of :305: fewer than half of the correspondences in front of both cameras */
  SVO_HIP_TWO_VIEW_FEW_INLIERS = 4    /* the gate of :85 */
};
#define SVO_HIP_TWO_VIEW_MAX_HYPOTHESES 4096
typedef struct {
  double reproj_thresh;               /* 2.0: Config::poseOptimThresh() (:81) */
  int min_inliers;                    /* 40: Config::initMinInliers() (:85) */
  double map_scale;                   /* 1.0: Config::mapScale() (:105) */
  int n_hypotheses;                   /* 1024; 1..SVO_HIP_TWO_VIEW_MAX_HYPOTHESES */
  unsigned long long seed;            /* 0 */
} svo_hip_two_view_params;
typedef struct {
  int status, n_in;
  int hypothesis, hypothesis_count;   /* the winner and its inlier count (-1, -1 before a model) */
  int candidate, candidate_count;     /* the chosen one of (R1, u3), (R1, -u3), (R2, u3), (R2, -u3) and its cheirality count */
  int n_inliers, n_points;            /* 0 unless status is OK: a failure leaves no inliers and no points (the reference
                                       * leaves the previous attempt's inliers_ in place at :307 -- not kept) */
  double depth_median, scale;         /* rank n_in / 2 of all xyz_in_cur.z (NaN if one of them is NaN); map_scale / median */
  double T_cur_from_ref[7];           /* T_f_w[7] layout; NaN before the cheirality gate is passed */
  double T_cur_w[7];                  /* the second frame's pose with the rescaled translation (:108-115); NaN unless OK */
} svo_hip_two_view_result;
int svo_hip_two_view_default_params(svo_hip_two_view_params* params);
/* computeFundamental and addSecondFrame :85-125 for the n listed cameras in one set of launches and one synchronisation.
 * cams[i] gives camera cameras[i] its errorMultiplier2 (|fx|) and its image size for the gate of :123; T_ref_w[i][7] is the
 * first frame's pose (NULL: identity for every camera, the reference's first frame); params may be NULL.  The KLT lists are
 * read, never written.  The handle's two-view memory is taken by its first call; later calls make no allocator call.  A
 * status other than OK is a result, not an error.  Before anything is enqueued: SVO_HIP_ERR_INVALID for a camera out of
 * range or listed twice, a camera model without size or focal length, reproj_thresh or map_scale not positive and finite,
 * min_inliers < 0, n_hypotheses outside 1..4096; SVO_HIP_ERR_STATE for a camera without a reference, or without a
 * svo_hip_klt_track / svo_hip_klt_set_lists since its reference was set (f_cur undefined).  A refused call leaves lists and
 * earlier results as they were. */
int svo_hip_klt_two_view(svo_hip_klt* klt, int n, const int* cameras, const svo_hip_camera* cams /*[n]*/,
                         const double* T_ref_w /*[n][7] or NULL*/, const svo_hip_two_view_params* params,
                         svo_hip_two_view_result* results /*[n]*/);
/* what the camera's last svo_hip_klt_two_view left on the device (xyz_in_cur_ and inliers_ of :82, the points of :119-125);
 * every output may be NULL.  status: the call's status again (it says which outputs are written); n: the correspondences; xyz_in_cur[n][3] (written for status OK and FEW_INLIERS only);
 * mask[n]: the winner's inlier flags (zeros before a model); inliers[n_inliers]; point_index[n_points]: the feature's position
 * in the camera's lists, in inlier order, with point_pos[n_points][3]; hypothesis_count[n_hypotheses]: every hypothesis' inlier
 * count, -1 for a degenerate sample (n_hypotheses = 0 for TOO_FEW).  SVO_HIP_ERR_STATE: no two-view call since the camera's
 * lists were last set.  Synchronises. */
int svo_hip_klt_download_two_view(svo_hip_klt* klt, int camera, int32_t* status, int32_t* n, double* xyz_in_cur, uint8_t* mask, int32_t* n_inliers,
                                  int32_t* inliers, int32_t* n_points, int32_t* point_index, double* point_pos,
                                  int32_t* n_hypotheses, int32_t* hypothesis_count);
/* the camera's lists from the host, for callers with a matcher of their own: px_ref[n][2], px_cur[n][2], f_ref[n][3],
 * f_cur[n][3] replace what trackKlt left (:203-225), index becomes 0..n-1, the disparities are undefined until the next
 * svo_hip_klt_track.  The camera must have a reference (SVO_HIP_ERR_STATE) and n <= max_features.  Synchronises. */
int svo_hip_klt_set_lists(svo_hip_klt* klt, int camera, int n, const float* px_ref, const float* px_cur, const double* f_ref,
                          const double* f_cur);

#ifdef __cplusplus
}
#endif
#endif /* SVO_HIP_H_ */
