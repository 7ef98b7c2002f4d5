/*
 * drt_hip.h -- C-ABI of the MI355X render launcher (libdrt_hip.so).
 *
 * This is the drop-in boundary for the per-pixel render loop of daily-ray-trace:
 * the host (plain C, POSIX) keeps loading .scn scenes and spectra CSVs exactly as
 * before, flattens them into the plain structs below, and calls drt_render_tile()
 * (or the drt_create/drt_render/drt_read_film session form) where the reference
 * runs its `for sample / for y / for x` loop.
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   - the pixel loop of render_image()           src/daily_ray_trace.c:710-745
 *   - sample_scene()                             src/daily_ray_trace.c:571-618
 *   - cast_ray() and everything below it         src/daily_ray_trace.c:215-479
 *   - the BDSF / direction-sampling plugin tables src/bdsf.h:1-52, src/bdsf_list.h
 *   - rng()/seed_rng()                           src/rng.h:1-2
 *   - spectrum_to_xyz()                          src/spectrum.c:49-70
 *
 * Everything here is plain C: pointers, sizes, doubles. No C++ or torch types.
 * All arithmetic on the path is IEEE f64; integers are u32/u64.
 *
 * The oracle (oracle/drt_oracle.h) consumes the SAME structs, so a parity test
 * hands one scene to both sides.
 */
#ifndef DRT_HIP_H
#define DRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRT_MAX_BDSFS 16 /* object_material.bdsfs[16], src/daily_ray_trace.h:109 */

/* Surface kinds keep the reference's numeric values (src/daily_ray_trace.h:7-14). */
enum
{
    DRT_GEO_NONE   = 0,
    DRT_GEO_POINT  = 1,
    DRT_GEO_SPHERE = 2,
    DRT_GEO_PLANE  = 3
};

/* film_sample_scheme, src/daily_ray_trace.h:20-26 */
enum
{
    DRT_FILM_SAMPLE_CENTER = 1,
    DRT_FILM_SAMPLE_RANDOM = 2
};

/*
 * Material plugin IDs. The names and their ORDER come from bdsf_list.h (the same
 * X-macro file the reference expands into function-pointer tables); here the list
 * expands to integer IDs because function pointers do not cross to the GPU.
 */
#define BDSF(name) DRT_BDSF_##name,
#define DIRF(name)
enum
{
#include "bdsf_list.h"
    DRT_NUM_BDSFS
};
#undef BDSF
#undef DIRF
#define BDSF(name)
#define DIRF(name) DRT_DIRF_##name,
enum
{
#include "bdsf_list.h"
    DRT_NUM_DIRFS
};
#undef BDSF
#undef DIRF

/* One surface: object_geometry (src/daily_ray_trace.h:78-93) without the name.
 * Planes carry the derived normal/u/v of create_plane_from_points (src/geometry.c:203-209). */
typedef struct drt_surface
{
    uint32_t type;     /* DRT_GEO_* */
    uint32_t material; /* index into drt_scene.materials */
    double   position[3];
    double   radius;   /* spheres */
    double   normal[3];
    double   u[3];
    double   v[3];
} drt_surface;

/* One material: object_material (src/daily_ray_trace.h:95-111). SPDs are indices into
 * drt_scene.spds; -1 means "not given" (a NULL spectrum in the reference) and reads as zeros. */
typedef struct drt_material
{
    uint32_t is_black_body;
    uint32_t is_emissive;
    double   shininess;
    double   roughness;
    int32_t  emission_spd;
    int32_t  diffuse_spd;
    int32_t  glossy_spd;
    int32_t  mirror_spd;
    int32_t  refract_spd;
    int32_t  extinct_spd;
    uint32_t num_bdsfs;
    uint32_t bdsfs[DRT_MAX_BDSFS]; /* DRT_BDSF_* */
    uint32_t dir_func;             /* DRT_DIRF_* */
} drt_material;

/* scene_data (src/daily_ray_trace.h:146-156) plus the spectral tables the path reads. */
typedef struct drt_scene
{
    uint32_t           num_surfaces;
    const drt_surface *surfaces;
    uint32_t           num_materials;
    const drt_material *materials;
    uint32_t           base_material;   /* scene_data.base_material   */
    uint32_t           escape_material; /* scene_data.escape_material */

    uint32_t      num_spds;
    uint32_t      num_wavelengths; /* number_of_spectrum_samples, src/spectrum.h:3 */
    const double *spds;            /* [num_spds][num_wavelengths] */
    double        min_wavelength;  /* smallest_wavelength (nm)     */
    double        wavelength_interval;
    /* colour-matching tables (cmfs, src/spectrum.h:17-23) as SPD indices */
    uint32_t cmf_rw, cmf_x, cmf_y, cmf_z;
} drt_scene;

/* camera_data, src/daily_ray_trace.h:158-170 -- same fields, same meaning. */
typedef struct drt_camera
{
    double forward[3];
    double right[3];
    double up[3];
    double aperture_position[3];
    double aperture_radius;
    double focal_depth;
    double focal_length;
    double film_bottom_left[3];
    double pixel_width;
    double pixel_height;
} drt_camera;

enum
{
    DRT_MODE_SPECTRAL = 0, /* film = sum(+filter), mean, variance per wavelength (the reference's output) */
    DRT_MODE_XYZ      = 1  /* XYZ-only film ("a different mode", reported as such): per pixel 8 doubles
                              {X, Y, Z numerators of wavelengths 0..63.., filter sum, X, Y, Z of the tail wavelengths, 0};
                              spectrum_to_xyz's sums are taken per kernel pair and added up, so no spectrum is kept, there
                              is no mean / variance, and 64 instead of 1664 bytes per pixel cross the links. In this mode
                              the "pixels" buffer of every call below is [tile_h*tile_w][8] and avgs / vars are NULL;
                              drt_read_xyz() gives the same XYZ as the spectral film's to rounding (order of sums). */
};

/*
 * What to render. The tile is the pixel set {(x0+i, y0+j*row_stride) : i<tile_w, j<tile_h} of a
 * width x height image (row_stride>1 gives the row-cyclic multi-GPU partition). Path RNG key
 * (SURVEY 8a-R): seed + ((sample*height + y)*width + x) as u64, xorshift64 seeded through splitmix64.
 */
typedef struct drt_params
{
    uint32_t width, height;
    uint32_t x0, y0, tile_w, tile_h, row_stride;
    uint32_t spp;          /* num_pixel_samples  */
    uint32_t first_sample; /* index of the first sample (resume support) */
    uint32_t max_depth;    /* max_cast_depth     */
    uint32_t pixel_scheme; /* DRT_FILM_SAMPLE_*  */
    uint64_t seed;
    uint32_t mode;         /* DRT_MODE_* */
    int32_t  device;       /* HIP device ordinal */
    uint32_t batch_spp;    /* samples traced per launch pair. 0 = sized for a job of `spp` samples (about 32 launch pairs, or as many samples
                              as about 16 GB of vertex records hold, whichever is more); DRT_BATCH_RESIDENT = sized for a context kept across
                              many frames (up to 256 M paths per launch, at least 16 samples per pixel, as memory allows) */
    uint32_t flags;        /* DRT_FLAG_* */
} drt_params;

#define DRT_BATCH_RESIDENT 0xFFFFFFFFu /* drt_params.batch_spp: let the library size launches for a long-lived context */

enum
{
    DRT_FLAG_RECORD_HITS = 1u, /* keep closest-hit surface indices per path vertex (parity tests) */
    DRT_FLAG_FILM_ZERO   = 2u  /* one-shot forms only: the caller's buffers are zero-filled (as the reference's alloc() leaves
                                  them, src/daily_ray_trace.c:689-691), so they are not uploaded before rendering */
};

typedef struct drt_stats
{
    uint64_t paths;
    uint64_t closest_hit_scans; /* find_ray_intersection calls (V_int)       */
    uint64_t shaded_vertices;   /* direct_light_contribution calls (V_shade) */
    uint64_t shadow_scans;      /* points_mutually_visible calls             */
    uint64_t rng_draws;
    double   trace_ms;          /* path-geometry kernel, HIP-event time      */
    double   shade_ms;          /* spectral shade + film kernel; while depth cuts, a sensor, buckets or lobes are bound (drt_bind_depth_cuts, drt_bind_sensor, drt_bind_buckets, drt_bind_lobes), that pass too */
    double   total_ms;
    /* the pool of vertex records (four vertices per block): its size, the most a launch has used, and how many launches had to be
     * rendered again in worst-case-sized pieces because the pool ran out (0 unless the tile's paths grew after the context measured them) */
    uint64_t record_pool_blocks;
    uint64_t record_pool_peak;
    uint32_t record_block_bytes;
    uint32_t redone_launches;
    /* the reference's per-pass report (min / max / avg time of one sample pass over the image, src/daily_ray_trace.c:746-756): a
     * kernel pair renders several samples of every pixel it covers, so a pair's HIP-event time is scaled to one sample of the
     * whole tile -- ms x tile pixels / (pixels x samples of the pair) -- and min / max / avg run over the pairs */
    uint32_t launches;   /* kernel pairs timed */
    uint32_t path_flags; /* which kernels this context runs: DRT_PATH_* (a group: the devices' flags or'ed) */
    double   min_sample_ms, max_sample_ms, avg_sample_ms;
} drt_stats;

enum
{
    DRT_PATH_BVH        = 1u, /* the scene is behind the bounding-volume hierarchy: drt_primary_kernel + drt_bounce_kernel trace it */
    DRT_PATH_TRACE_TAIL = 2u, /* the trace kernel carries every path's tail wavelengths (all-plastic scenes); the shade kernel's tail pass only updates the film */
    DRT_PATH_RAYS       = 4u, /* a ray table is bound (drt_bind_rays): the ray-mode entry points of those kernels run; set while bound, and only then */
    DRT_PATH_RAY_STASH  = 8u  /* the context's camera launches start their paths from the trace kernel's ray stash (drt_trace_kernel); unset: from the direct
                                 start (drt_trace_direct_kernel: DRT_NO_RAY_STASH=1, or an LDS block without room for the stash) or in the hierarchy's
                                 kernels. A property of the context like the two above: while DRT_PATH_RAYS is set the ray-mode kernels run instead,
                                 and those start directly */
};

typedef struct drt_context drt_context;

/* Last error text of the calling thread ("" when none). */
const char *drt_last_error(void);
/* Number of HIP devices visible; negative on error. */
int drt_device_count(void);

/* Session form. drt_create copies the scene to the device (SoA) and allocates the film
 * (zero-filled, like the reference's VirtualAlloc'ed accumulators, src/daily_ray_trace.c:689-691). */
drt_context *drt_create(const drt_scene *scene, const drt_camera *camera, const drt_params *params);
void         drt_destroy(drt_context *ctx);
/* Use caller-owned DEVICE buffers for the film instead of the library's own
 * ([tile_h*tile_w][S+1], [..][S], [..][S] doubles). The caller zero-fills them. */
int drt_bind_film(drt_context *ctx, void *d_pixels, void *d_avgs, void *d_vars);
/* Launch on this hipStream_t (NULL = the context's own stream). */
int drt_set_stream(drt_context *ctx, void *hip_stream);
/* Enqueue samples [first_sample, first_sample+num_samples) for every tile pixel. Asynchronous. */
int drt_render(drt_context *ctx, uint32_t first_sample, uint32_t num_samples);
int drt_synchronize(drt_context *ctx);
/* Zero the film and the statistics (for repeated timed runs). */
int drt_reset_film(drt_context *ctx);
/* Device pointers of the film buffers (for collectives on them). */
int drt_film_device_ptrs(drt_context *ctx, void **d_pixels, void **d_avgs, void **d_vars);
/* Copy the film to host buffers (any may be NULL). Synchronises. */
int drt_read_film(drt_context *ctx, double *pixels, double *avgs, double *vars);
/* Replace the film with host data (any pointer may be NULL to leave that buffer as is): resuming from a checkpoint. */
int drt_write_film(drt_context *ctx, const double *pixels, const double *avgs, const double *vars);
/* Per-pixel XYZ of sum/filter (spectrum_to_xyz on the device), [tile_h*tile_w][3]. Synchronises. */
int drt_read_xyz(drt_context *ctx, double *xyz);
/* One film buffer as the pixel bytes of the reference's .bmp outputs, [tile_h*tile_w][4] = B, G, R, 255, tile row 0 first (the
 * order a bottom-up BMP stores them): which = 0 sum / filter, 1 running mean, 2 variance / its largest sample. Replaces
 * spd_file_to_rgb_f64_pixels (src/daily_ray_trace.c:1-28) + spectrum_to_rgb_f64 (src/spectrum.c:72-82) + rgb_f64_to_rgb_u8
 * (src/win32_platform.c:136-147) with one kernel over the resident film. DRT_MODE_SPECTRAL only. Synchronises. */
int drt_read_bgra(drt_context *ctx, int which, uint8_t *bgra);
/* Closest-hit surface indices of the LAST rendered sample batch: [n][max_depth] int32 per path
 * (-1 miss, -2 vertex not reached); needs DRT_FLAG_RECORD_HITS. Paths are ordered
 * (sample - first_sample_of_last_call, tile row, tile column). */
int drt_read_hit_indices(drt_context *ctx, int32_t *dst, uint64_t capacity_paths);
int drt_get_stats(drt_context *ctx, drt_stats *out);
/* Samples per pixel one trace+shade kernel pair processes (the launch granularity); 0 on error. */
uint32_t drt_batch_spp(drt_context *ctx);

/* Which instantiation of the shade kernel the context's dense launches run (read-only; -1: ctx is null). GENERAL has the general BDSF
 * list; SIMPLE is for scenes that list nothing but bp_diffuse_bdsf, bp_glossy_bdsf and mirror_bdsf; CLOSED is for scenes whose every
 * material lists nothing or exactly one of the lists that have straight-line code (two-lobe plastic, mirror, glass pair, smooth
 * conductor, rough conductor) and no surface has a material that is no black body and lists nothing, on a spectral film with one wavelength set per lane and the SPD table in LDS. Decided when the context
 * is created (DRT_NO_SIMPLE_SHADE, DRT_NO_CLOSED_SHADE and DRT_NO_FIXED_LISTS are read there); material updates keep every list, so it
 * holds for the context's life. All three compute the same film, bit for bit. */
#define DRT_SHADE_GENERAL 0
#define DRT_SHADE_SIMPLE 1
#define DRT_SHADE_CLOSED 2
int drt_shade_instantiation(const drt_context *ctx);
/* 1: the context's dense launches run the closed instantiation's form with window headers in LDS, five waves per SIMD
 * (drt_shade_kernel_closed_lds); 0: any other kernel; -1: null context */
int drt_shade_closed_lds(const drt_context *ctx);
/* waves per SIMD of the closed kernel the context's dense launches run: 6 (drt_shade_kernel_closed_lds6: 512-lane workgroups, one SPD
 * table for eight waves; DRT_CLOSED_WAVES=5 at creation keeps the five-wave kernel), 5, 4; 0: another instantiation; -1: null context */
int drt_shade_closed_waves(const drt_context *ctx);

/*
 * One-shot form matching the reference's loop: host buffers, caller-owned,
 * accumulated INTO (so the caller zero-fills them, as alloc() does in the reference).
 * Returns 0 on success, negative on failure (see drt_last_error()).
 */
int drt_render_tile(const drt_scene *scene, const drt_camera *camera, const drt_params *params,
                    double *dst_pixels, double *dst_avgs, double *dst_vars, drt_stats *stats);

/*
 * Several GPUs from ONE host thread (SURVEY 8b "Threading": the launcher may drive 1..8 devices, one stream each).
 * The tile's rows are dealt cyclically over the devices -- device k of n owns tile rows k, k+n, ... for all samples,
 * the same partition the multi-process callers use -- each device has its own context and stream, all of them render
 * concurrently, and the film comes back into the caller's buffers in image order (one strided copy per device and
 * buffer). `devices` lists HIP device ordinals (a device may appear more than once: that many contexts share it);
 * devices == NULL means 0..n_devices-1, n_devices == 0 means every visible device; drt_params.device is ignored.
 * Results are bit-identical to a single context's, whatever the device list.
 */
typedef struct drt_group drt_group;
drt_group *drt_group_create(const drt_scene *scene, const drt_camera *camera, const drt_params *params,
                            const int32_t *devices, uint32_t n_devices);
void     drt_group_destroy(drt_group *g);
uint32_t drt_group_size(drt_group *g);
/* Enqueue samples [first_sample, first_sample+num_samples) on every device. Asynchronous. */
int drt_group_render(drt_group *g, uint32_t first_sample, uint32_t num_samples);
int drt_group_synchronize(drt_group *g);
/* Whole-tile film buffers ([tile_h*tile_w][S+1], [..][S], [..][S]) <-> the devices' row sets. NULL skips a buffer. */
int drt_group_read_film(drt_group *g, double *pixels, double *avgs, double *vars);
int drt_group_write_film(drt_group *g, const double *pixels, const double *avgs, const double *vars);
int drt_group_read_bgra(drt_group *g, int which, uint8_t *bgra); /* drt_read_bgra over the whole image */
/* Counters summed over the devices; trace_ms / shade_ms / total_ms are the slowest device's. */
int drt_group_get_stats(drt_group *g, drt_stats *out);
/* One-shot form of drt_render_tile over a device list. */
int drt_render_tile_multi(const drt_scene *scene, const drt_camera *camera, const drt_params *params,
                          const int32_t *devices, uint32_t n_devices,
                          double *dst_pixels, double *dst_avgs, double *dst_vars, drt_stats *stats);

/*
 * Adaptive sampling: stop sampling pixels whose film has converged. Round 0 renders samples [0, min_spp) of every tile pixel; each
 * later round the next min(step, max_spp - n) samples of every pixel still active (all of them hold the same n). After a round each
 * pixel rendered in it is tested on its own film (c = n samples; rw, cy the rows cmf_rw, cmf_y; avg, var its film rows):
 *     N = interval * sum_i cy[i] rw[i]
 *     Y = (sum_i cy[i] avg[i] rw[i]) * (interval / N),  E = (sum_i cy[i] sqrt(var[i] / (c (c - 1))) rw[i]) * (interval / N)
 *     active next round  <=>  n < max_spp  &&  !(E <= rel_error * max(|Y|, floor))
 * (sums sequential over ascending i, no contraction; a NaN stays active until max_spp). A pixel that ends with n_p samples holds,
 * bit for bit, the film a uniform n_p-sample render gives it; the filter column of the film is its count.
 */
typedef struct drt_adaptive
{
    uint32_t min_spp, max_spp, step, flags; /* min_spp >= 2, max_spp >= min_spp, step >= 1; flags: 0 (reserved) */
    double   rel_error, floor;              /* finite, rel_error > 0, floor >= 0 */
    uint32_t rounds, pixels_at_max;         /* out */
    uint64_t paths;                         /* out: samples rendered, summed over pixels */
} drt_adaptive;                             /* 48 bytes */
/* Synchronous. Needs a film without samples (a fresh context, or drt_reset_film after drt_render / drt_write_film), DRT_MODE_SPECTRAL and
 * no DRT_FLAG_RECORD_HITS; refuses (nonzero, drt_last_error, nothing rendered) otherwise or on inputs out of range. Afterwards
 * drt_render, drt_write_film and another adaptive call are refused until drt_reset_film. drt_get_stats counts every round. */
int drt_render_adaptive(drt_context *ctx, drt_adaptive *a);
/* Samples per pixel of the last adaptive render, [tile_h*tile_w]. Synchronises. */
int drt_read_sample_counts(drt_context *ctx, uint32_t *counts);
/* The pixels (tile indices, ascending) still active after the last round of the last adaptive render -- none once it has run to the
 * end; the test knob DRT_ADAPTIVE_ROUNDS=k stops a render after k rounds. *count gets their number; capacity smaller than that is an
 * error. Synchronises. */
int drt_read_active_list(drt_context *ctx, uint32_t *list, uint32_t capacity, uint32_t *count);
/* The group forms: every device runs its own rounds on its rows; film and counts are the same for any device list. */
int drt_group_render_adaptive(drt_group *g, drt_adaptive *a);
int drt_group_read_sample_counts(drt_group *g, uint32_t *counts); /* whole tile, image order */

/*
 * Continue adaptive sampling on the film the context HOLDS: whatever drt_render, drt_write_film, drt_render_adaptive or an earlier
 * call of this function left there. The rule above holds per pixel, with the pixel's own count n_p where it says n: pixel p's count is
 * its filter sum, c = n_p in E, p is active iff n_p < max_spp && !(E <= rel_error * max(|Y|, floor)), and an active pixel's next
 * allotment is min(step, max_spp - n_p). First every pixel is tested on its own rows (nothing is rendered); then rounds as in
 * drt_render_adaptive over the pixels that stay active, each rendering samples [n_p, n_p + min(step, max_spp - n_p)) of pixel p.
 * max_rounds = 0: until no pixel is active; k: return after at most k rendering rounds. a->min_spp is not used (checked as in
 * drt_render_adaptive, nothing more). A pixel with n_p >= max_spp is finished.
 * Out: a->rounds rendering rounds run by THIS call, a->paths samples rendered by this call, a->pixels_at_max tile pixels with
 * n_p >= max_spp at return; *still_active (may be NULL) the length of the active list at return.
 * Afterwards the context is in the state an adaptive render leaves (drt_read_sample_counts, drt_read_active_list, drt_read_film and
 * drt_read_bgra work; drt_render and drt_write_film are refused until drt_reset_film), and the call may be repeated, with the same
 * or other parameters. Continuing with a rel_error and floor no larger and a max_spp no smaller than before (same step, same grid of
 * counts) gives the film and the counts of one drt_render_adaptive call with the new parameters; drt_render(0, m) followed by this
 * call those of drt_render_adaptive with min_spp = m.
 * Refused (nonzero, drt_last_error, nothing rendered, no film bit changed): DRT_MODE_XYZ, DRT_FLAG_RECORD_HITS, inputs out of range, a
 * film without samples, a filter sum that is not a whole number in [2, 2^32) (the message names the first such tile pixel), and the
 * allotment contract: a round renders the same number of samples of every active pixel, so after the first test either all active
 * pixels hold the same count (the rounds are then drt_render_adaptive's, a partial last round included) or every active pixel's
 * max_spp - n_p is a multiple of step (every round then renders step samples of each). The rounds keep either property. The message of
 * that refusal lists the values of step that would do. In the group form the contract is decided over the whole tile, and parameters,
 * films and contract are checked on all devices before any device renders; film, counts and report are the same for any device list.
 */
int drt_render_adaptive_continue(drt_context *ctx, drt_adaptive *a, uint32_t max_rounds, uint32_t *still_active);
int drt_group_render_adaptive_continue(drt_group *g, drt_adaptive *a, uint32_t max_rounds, uint32_t *still_active);

/*
 * Sample maps: render every tile pixel to a sample count the caller gives. targets[p] belongs to tile pixel p (tile order). Pixel p's
 * count n_p is its filter sum, a whole number in [0, 2^32): 0 and 1 are counts here, and a fresh film holds 0 everywhere.
 *     absolute mode (flags 0):  R_p = targets[p] > n_p ? targets[p] - n_p : 0     (a pixel above its target is left alone)
 *     DRT_MAP_ADD:              R_p = targets[p]                                  (n_p + targets[p] must not pass 2^32 - 1)
 * The call renders samples [n_p, n_p + R_p) of every pixel in binary rounds: with B the OR of all R_p, one round per set bit b of B
 * in ascending order, which renders the next 2^b samples of every pixel whose R_p has bit b, each from the count it holds then, the
 * round's pixels listed in ascending tile order. A remainder of 5 is 1 sample in round 0 and 4 in round 2; there are at most 32 rounds.
 * Afterwards pixel p holds, bit for bit in all three buffers, the film of a uniform render of samples [0, n_p + R_p).
 * Out: rounds = popcount(B); paths = sum of R_p; pixels_rendered = pixels with R_p > 0; pixels_above = pixels with n_p > targets[p]
 * (absolute mode; 0 with DRT_MAP_ADD); max_count = the largest count after the call.
 * DRT_MAP_DEVICE: targets is device memory on the context's device, read by a kernel on the context's stream and never copied to the
 * host; without it targets is host memory. Synchronous.
 * Afterwards the context is in the state an adaptive render leaves, with an empty active list: drt_read_sample_counts,
 * drt_read_active_list (0 entries), drt_read_film, drt_read_bgra, drt_read_xyz, drt_denoise_film, drt_render_features and
 * drt_render_mattes with n_samples = 0 (under their own count rules), drt_render_adaptive_continue (under its own rules) and another
 * drt_render_sample_map work; drt_render and drt_write_film are refused until drt_reset_film. A map that asks for nothing succeeds
 * with 0 rounds and leaves the same state.
 * Refused (nonzero, drt_last_error, nothing rendered, no film bit changed): a null pointer, undefined flag bits, bound depth cuts, a bound
 * sensor,
 * DRT_MODE_XYZ, DRT_FLAG_RECORD_HITS, a tile of more than 2^32 - 1 pixels, a filter sum that is not a whole number in [0, 2^32) and a
 * DRT_MAP_ADD overflow (either message names the first such tile pixel), and a failed allocation.
 * The group form takes host memory only (DRT_MAP_DEVICE is refused): the whole tile in image order, every device its own rows. All
 * checks, the adoption included, run on all devices before any device renders; rounds = popcount of the OR over all devices, the sums
 * and the maximum are taken over all devices; film, counts and report are the same for any device list.
 */
#define DRT_MAP_DEVICE 1u
#define DRT_MAP_ADD    2u
typedef struct drt_sample_map
{
    const uint32_t *targets;            /* [tile_h*tile_w] */
    uint32_t flags;
    uint32_t rounds, pixels_rendered, pixels_above, max_count;  /* out */
    uint64_t paths;                                             /* out */
} drt_sample_map;                       /* 40 bytes */
int drt_render_sample_map(drt_context *ctx, drt_sample_map *map);
int drt_group_render_sample_map(drt_group *g, drt_sample_map *map);

/*
 * Variance-guided denoising of the spectral film. The film holds, per pixel and wavelength, a running mean and a sum of squared
 * deviations, and in its filter column the sample count c: what is left after a render is noise of known size. The filter is a
 * non-local mean over a (2 radius + 1)^2 window whose weights compare (2 patch + 1)^2 patches of the pixels' XYZ against the
 * variance of that XYZ, gated by the centre pair's own distance; DESIGN.md section 5b states the rule, which uses + - * / sqrt
 * only, and tests/denoise_rule.py restates it in numpy: the device's result equals that bit for bit. A pixel is usable when its count
 * is a whole number in [2, 2^32) and its guide values are finite; an unusable pixel passes through (mean' = mean, var' = var / (c (c - 1)))
 * and weighs nothing anywhere else.
 *   mean'[p][i] = sum_q w(p,q) avg[q][i] / W,   var'[p][i] = sum_q w(p,q)^2 (var[q][i] / (c_q (c_q - 1))) / W^2,   W = sum_q w(p,q)
 */
typedef struct drt_denoise
{
    uint32_t radius, patch, flags; /* radius 0..10, patch 0..3; flags: 0 (reserved). Suggested: 5, 1 */
    uint32_t unusable;             /* out: pixels that passed through */
    double   k, alpha;             /* finite, k > 0, alpha >= 0. Suggested: 1, 1 */
    double   kernel_ms;            /* out: HIP-event time of the three kernels */
} drt_denoise;                     /* 40 bytes */
/* Filters the film the context holds -- after drt_render, drt_write_film or either adaptive call -- into two buffers of the context's
 * own. Synchronises first. Changes no film bit, no count and no render state: drt_render continues afterwards as if it had not been
 * called. Refused with nothing done: parameters out of range (checked before any device call), DRT_MODE_XYZ, row_stride != 1. */
int drt_denoise_film(drt_context *ctx, drt_denoise *d);
/* The result of the last drt_denoise_film, [tile_h*tile_w][S] each; either pointer may be NULL. An error before a drt_denoise_film, and
 * after anything has changed the film since (drt_render, drt_write_film, drt_reset_film, drt_bind_film, an adaptive call). */
int drt_read_denoised(drt_context *ctx, double *mean, double *var);
/* The denoised mean as .bmp pixel bytes: the conversion of drt_read_bgra(ctx, 1, ...) applied to mean'. Same errors. */
int drt_read_denoised_bgra(drt_context *ctx, uint8_t *bgra);
/* One-shot on host buffers of a whole tile_w x tile_h film (also the post-process of a stored .spd triplet), on params->device; of
 * params only tile_w, tile_h, row_stride, mode and device are read. d is in-out. mean or var may be NULL. */
int drt_denoise_buffers(const drt_scene *scene, const drt_params *params, drt_denoise *d, const double *pixels, const double *avgs,
                        const double *vars, double *mean, double *var);
/* Row-cyclic devices hold no neighbours of their own rows: the group gathers its film as drt_group_read_film does and runs the one-shot
 * form on its first device. Same bits for any device list. */
int drt_group_denoise(drt_group *g, drt_denoise *d, double *mean, double *var);

/*
 * First-hit feature buffers: what a pixel looks at. Per tile pixel p with count c_p, and for sample s = first_sample .. first_sample + c_p - 1
 * in ascending order: the path's own camera ray (the RNG seeded with the path key of (x, y, s), then the draws the render takes, in its
 * order), its closest hit as the render finds it (fudged origin, facing normal after the flip), and of that the vector phi of
 * DRT_FEATURE_CHANNELS doubles:
 *     phi[0..2] the hit normal,  phi[3] the depth (position - aperture_position) . forward,  phi[4] 1,  phi[5..7] the XYZ of the surface material
 *     a miss (a NaN ray misses): phi[0..4] = 0, phi[5..7] the XYZ of the escape material
 * A material's XYZ is that of its emission when it is emissive, else of (diffuse + glossy) + mirror (an SPD index of -1 reads as zeros),
 * channel k with colour-matching row ck being (sum_i ck[i] r[i] rw[i]) * (interval / N), N as in drt_adaptive above. Every channel is
 * updated the way the film is (src/daily_ray_trace.c:736-743): d = phi - m; m = m + d / (double)(s - first_sample + 1); M2 = M2 + d * (phi - m).
 * Results: mean [tile_h*tile_w][DRT_FEATURE_CHANNELS], m2 likewise (not divided, like the film's variance: mean[..][4] is the coverage),
 * ids [tile_h*tile_w], the closest-hit surface index of sample first_sample (-1 for a miss). DESIGN.md section 5c states the rule, which
 * uses + - * / sqrt only, and tests/feature_rule.py restates it: the device's result equals that bit for bit.
 */
#define DRT_FEATURE_CHANNELS 8
typedef struct drt_features
{
    uint32_t n_samples;    /* >0: that many samples of every pixel; 0: each pixel's count from the held film's filter column */
    uint32_t first_sample;
    uint32_t flags;        /* 0 (reserved) */
    uint32_t empty_pixels; /* out: pixels whose coverage is 0 */
    uint64_t rays;         /* out: camera rays cast, summed over pixels */
    double   kernel_ms;    /* out: HIP-event time */
} drt_features;            /* 32 bytes */
/* Synchronises, then fills three buffers of the context's own. Changes no film bit, no count and no render state: drt_render and the
 * adaptive calls go on afterwards as if it had not been called. n_samples > 0 works in both film modes and on an empty film. n_samples = 0
 * needs DRT_MODE_SPECTRAL and a film whose every filter sum is a whole number in [1, 2^32). Refused with nothing done: nonzero flags,
 * first_sample + count beyond 2^32 - 1, and with n_samples = 0 the XYZ film and a filter sum that is no count (the message names the
 * first such tile pixel). */
int drt_render_features(drt_context *ctx, drt_features *f);
/* The result of the last drt_render_features; any pointer may be NULL. An error before a drt_render_features, and -- when that call took
 * its counts from the film (n_samples = 0) -- after anything has changed the film since (drt_render, drt_write_film, drt_reset_film,
 * drt_bind_film, an adaptive call). */
int drt_read_features(drt_context *ctx, double *mean, double *m2, int32_t *ids);
/* One feature of the mean as .bmp pixel bytes, [tile_h*tile_w][4] = B, G, R, 255 in drt_read_bgra's row order: which = 0 the normal
 * (x, y, z to R, G, B), 1 the depth, 2 the coverage (both grey). t = (v - lo) / (hi - lo); t = t < 0 ? 0 : t; t = t > 1 ? 1 : t;
 * byte = (uint8_t)(t * 255.0 + 0.5); a NaN gives 0. Refused: hi <= lo, or either not finite; drt_read_features' errors. */
int drt_read_feature_bgra(drt_context *ctx, int which, double lo, double hi, uint8_t *bgra);
/* Features need no neighbours: every device renders its own rows, and the host buffers (whole tile, any may be NULL) come back in image
 * order. Same bits for any device list. With n_samples = 0 every device checks its film before any device renders. kernel_ms is the
 * slowest device's. */
int drt_group_render_features(drt_group *g, drt_features *f, double *mean, double *m2, int32_t *ids);

/*
 * ID mattes: which surface, and which material, a pixel shows, and how much of each. The samples are the feature pass's: per tile pixel p
 * with count c_p, sample s = first_sample .. first_sample + c_p - 1 in ascending order, the path's own camera ray and its closest hit. A
 * hit has a surface id, the closest-hit index, and a material id, that surface's material index; a miss (a NaN ray misses) has neither.
 * Two layers, DRT_MATTE_SURFACE and DRT_MATTE_MATERIAL, each of DRT_MATTE_SLOTS slots of (id, count), all empty at the start. A miss adds
 * 1 to `misses` (one number for both layers). A hit does in each layer, with that layer's id: a slot that holds the id gets count + 1;
 * else the lowest empty slot takes (id, 1); else other[layer] gets + 1. So the order of the samples matters only to a pixel that sees
 * more than DRT_MATTE_SLOTS ids. After the last sample each layer's slots are ranked by count descending, then id ascending, the empty
 * ones last as (DRT_MATTE_ID_MISS, 0). For every pixel and layer sum(counts) + other + misses == c_p.
 * Results: ids [tile_h*tile_w][DRT_MATTE_LAYERS][DRT_MATTE_SLOTS], counts likewise, tail [tile_h*tile_w][4] = c_p, misses, the surface
 * layer's other, the material layer's other. DESIGN.md section 5d states the rule and tests/matte_rule.py restates it: integers only,
 * and the device's result equals that.
 */
#define DRT_MATTE_SLOTS   6
#define DRT_MATTE_ID_MISS (-1)
enum { DRT_MATTE_SURFACE = 0, DRT_MATTE_MATERIAL = 1, DRT_MATTE_LAYERS = 2 };
typedef struct drt_mattes
{
    uint32_t n_samples;          /* >0: that many samples of every pixel; 0: each pixel's count from the held film's filter column */
    uint32_t first_sample;
    uint32_t flags;              /* 0 (reserved) */
    uint32_t empty_pixels;       /* out: pixels with misses == c_p */
    uint32_t overflow_pixels[2]; /* out: pixels with other > 0, per layer */
    uint64_t rays;               /* out: camera rays cast, summed over pixels */
    double   kernel_ms;          /* out: HIP-event time */
} drt_mattes;                    /* 40 bytes */
/* Synchronises, then fills three buffers of the context's own. Changes no film bit, no count, no render state and no feature buffer:
 * drt_render and the adaptive calls go on afterwards as if it had not been called. n_samples > 0 works in both film modes and on an empty
 * film. n_samples = 0 needs DRT_MODE_SPECTRAL and a film whose every filter sum is a whole number in [1, 2^32). Refused with nothing
 * done: nonzero flags, first_sample + count beyond 2^32 - 1, and with n_samples = 0 the XYZ film and a filter sum that is no count (the
 * message names the first such tile pixel). */
int drt_render_mattes(drt_context *ctx, drt_mattes *m);
/* The result of the last drt_render_mattes; any pointer may be NULL. An error before a drt_render_mattes, and -- when that call took its
 * counts from the film (n_samples = 0) -- after anything has changed the film since (drt_render, drt_write_film, drt_reset_film,
 * drt_bind_film, an adaptive call). */
int drt_read_mattes(drt_context *ctx, int32_t *ids, uint32_t *counts, uint32_t *tail);
/* One matte, [tile_h*tile_w]: coverage[p] = (double)(sum of count_k over the layer's slots whose id is in id_list) / (double)c_p, the sum
 * taken in integers; DRT_MATTE_ID_MISS in the list adds misses. Refused: layer not 0 or 1, n_ids of 0 or above 4096, an id below -1, an
 * id not below the scene's surface count (layer 0) or material count (layer 1); drt_read_mattes' errors. */
int drt_read_matte(drt_context *ctx, int layer, const int32_t *id_list, uint32_t n_ids, double *coverage);
/* A preview of one layer as .bmp pixel bytes, [tile_h*tile_w][4] = B, G, R, 255 in drt_read_bgra's row order. An id's colour:
 * h = (uint32_t)(id + 1) * 0x9E3779B1u; h ^= h >> 16; (R, G, B) = 64 + (h & 127), 64 + ((h >> 8) & 127), 64 + ((h >> 16) & 127). Per channel
 * v = sum over the ranked slots, from +0, of ((double)count_k / (double)c_p) * (double)colour(id_k); byte = (uint8_t)(v + 0.5), which is
 * 191 at most. Misses and `other` add nothing. Refused: layer not 0 or 1; drt_read_mattes' errors. */
int drt_read_matte_bgra(drt_context *ctx, int layer, uint8_t *bgra);
/* As drt_group_render_features: every device renders its own rows, and the host buffers (whole tile, any may be NULL) come back in image
 * order. Same bits for any device list. Every device is checked before any device renders. The out fields are summed over the devices;
 * kernel_ms is the slowest device's. */
int drt_group_render_mattes(drt_group *g, drt_mattes *m, int32_t *ids, uint32_t *counts, uint32_t *tail);

/*
 * Ray queries: the two questions the whole path is built on, asked of the resident scene for rays the caller supplies. The reference's
 * find_ray_intersection (src/daily_ray_trace.c:334-403) and points_mutually_visible (:238-270) are the rule, and the oracle's
 * restatement of them is what the device's answers equal bit for bit; DESIGN.md section 5e.
 *
 * A query reads the scene tables and the camera only: it changes no film bit, count, statistic, hit log, record pool, feature or matte
 * buffer and no film generation count, and may be issued between two drt_render calls. n = 0 is a successful no-op. Refused with a
 * message in drt_last_error() and no device call: a null required pointer when n > 0, flags other than DRT_RAYS_DEVICE, n above 2^31 in
 * device mode, and (host mode) a pixel outside the image. Host mode (flags = 0: all pointers are host memory) goes through staging
 * buffers of about a million rays, chunk by chunk, and synchronises the context's stream before it returns. Device mode
 * (DRT_RAYS_DEVICE) enqueues one launch on the context's stream (drt_set_stream) and returns without waiting: drt_synchronize or the
 * caller's own stream order completes it. There the host cannot read xy: a pixel outside the image gets a NaN ray, which misses.
 * In a context whose scene is behind the hierarchy (DRT_PATH_BVH) the box tests' error budget covers origins within the extent the
 * hierarchy was built for (the scene and the camera); origins far outside it are not held to the rule.
 * Directions in a DRT_PATH_BVH context: the hierarchy walk is derived for |d| = 1, and the rule is not the geometric answer otherwise
 * (line_sphere_intersection sets a = 1 whatever |d| is). drt_cast_rays keeps the rule bit for bit all the same: a ray whose finite
 * direction has | d.d - 1 | > 2^-42 is answered by the reference's own loop over ALL surfaces, so it costs a scan of the whole scene
 * instead of a walk (anything normalised in f64 is far inside the tolerance). NaN and infinite directions walk, and miss; for an
 * infinite component the rule can answer a hit at -inf, so behind the hierarchy infinite directions are not held to the rule.
 * drt_test_visibility normalises its own directions; drt_cast_pixels casts the camera's.
 */
typedef struct drt_ray_hit /* scene_point, src/daily_ray_trace.h:113-125, plus the distance */
{
    double   position[3], normal[3], out[3]; /* moved origin + dir * distance; the facing normal after the flip (:388-394); -dir */
    double   on_dot;                         /* normal . out, as :379 and :393 compute it */
    double   distance;                       /* min_dist: measured from the origin AFTER it was moved by vis_fudge (:339) */
    int32_t  index;                          /* closest-hit surface index, -1: a miss */
    uint32_t surface_material, incident_material, transmit_material; /* :381-395: a sphere entered from inside swaps the two media, a plane does not */
} drt_ray_hit;                               /* 104 bytes, no padding. A miss: index -1, surface_material the escape material, the rest +0 / 0 */

#define DRT_RAYS_DEVICE 1u /* all pointers are device memory on the context's device */

/* find_ray_intersection (src/daily_ray_trace.c:334-403) of ray i = (origins[i], dirs[i]), each [n][3]: the origin is moved by vis_fudge
 * along dirs[i] as given (no normalisation, :339), the comparison is a strict < over ascending surfaces (:340-364). A NaN direction misses. */
int drt_cast_rays(drt_context *ctx, const double *origins, const double *dirs, uint64_t n, drt_ray_hit *hits, uint32_t flags);
/* points_mutually_visible (src/daily_ray_trace.c:238-270) of (p0[i], p1[i]), each [n][3]: visible[i] is 1 or 0. The direction is normalised
 * (:241), the origin moved by the fudge (:242), the limit |p1 - o| - fudge (:243). p0 == p1 gives a NaN direction and the reference's answer to it. */
int drt_test_visibility(drt_context *ctx, const double *p0, const double *p1, uint64_t n, uint8_t *visible, uint32_t flags);
/* Query i is pixel (xy[2i], xy[2i+1]) of the whole width x height image (not only the context's tile) and sample samples[i]: the path's
 * own camera ray (sample_scene's ray set-up, src/daily_ray_trace.c:550-607, seeded with the path key), written to origins / dirs where
 * those are not null, and its closest hit as drt_cast_rays gives it. hits[i].index is drt_read_hit_indices' column 0 of that path. */
int drt_cast_pixels(drt_context *ctx, const uint32_t *xy, const uint32_t *samples, uint64_t n, double *origins, double *dirs, drt_ray_hit *hits,
                    uint32_t flags);
/* Host pointers only. The list is split into contiguous shares, one per device; results come back in list order; everything is checked
 * before any launch. Same bits as one context for any device list. */
int drt_group_cast_rays(drt_group *g, const double *origins, const double *dirs, uint64_t n, drt_ray_hit *hits);
int drt_group_test_visibility(drt_group *g, const double *p0, const double *p1, uint64_t n, uint8_t *visible);
int drt_group_cast_pixels(drt_group *g, const uint32_t *xy, const uint32_t *samples, uint64_t n, double *origins, double *dirs, drt_ray_hit *hits);

/*
 * Ray films: the path's FIRST ray as an input. A context bound to a ray table renders, per image pixel and sample, the spectral radiance
 * that arrives along a ray the caller supplies, where sample_scene makes one from the pinhole / thin-lens camera
 * (src/daily_ray_trace.c:577-607, camera_ray :550-607) and weighs it by the vignette (:614). Everything below the first ray -- cast_ray,
 * the RNG keys, the film update, the shade kernel -- is unchanged; DESIGN.md section 5f.
 *
 * The table has n_layers >= 1 layers over the WHOLE width x height image (not only the context's tile):
 *     origins[n_layers][height][width][3], dirs[n_layers][height][width][3], weights[n_layers][height][width] (NULL: every weight 1.0).
 * For image pixel (x, y) and absolute sample index s (first_sample, and in adaptive rounds the pixel's own count, included):
 *     l = s % n_layers,  r = (l * height + y) * width + x   (64-bit);
 *     the RNG is seeded from the path key seed + ((s * height + y) * width + x) as always, and NO draw is taken before cast_ray;
 *     ray_origin = origins[r], ray_direction = dirs[r] as given (no normalisation, as drt_cast_rays); cast_ray runs unchanged;
 *     the contribution is multiplied by weights[r] * 1.0 where :614-615 multiply by vignette_factor * pixel_filter_value.
 * A NaN direction misses: the pixel gets what an escaping ray leaves. A NaN weight makes its own pixel NaN and no other.
 *
 * flags = 0 (host mode): the arrays are host memory; the context copies the rows of its own tile (x0, y0, tile_w, tile_h, row_stride) of
 * every layer to its device before the call returns, and the caller's arrays are free afterwards. DRT_RAYS_DEVICE: the arrays are
 * whole-image arrays on the context's device, used in place -- no copy, no wait -- and must outlive the binding.
 * t == NULL unbinds: the context renders through its camera again.
 *
 * Binding and unbinding need a film without samples (a fresh context, or after drt_reset_film). Otherwise, and for null origins or dirs,
 * n_layers == 0, flags other than DRT_RAYS_DEVICE, or device mode in the group form, the call is refused with a message in
 * drt_last_error(): nothing is changed, no film bit included. While a table is bound drt_render, the adaptive calls, the film reads and
 * writes, the XYZ mode, the hit log, the denoiser, drt_cast_rays and drt_test_visibility work as before; drt_render_features,
 * drt_render_mattes, drt_cast_pixels and their group forms are refused, since they ask for the camera's rays. drt_stats.path_flags
 * carries DRT_PATH_RAYS while a table is bound. As for the ray queries, in a DRT_PATH_BVH context the box tests' error budget covers origins
 * within the extent the hierarchy was built for (the scene and the context's camera). Directions there: a first direction keeps its
 * length through mirror and glass vertices into the hierarchy walk, which is derived for |d| = 1, and the path has no scan to fall
 * back on. So in a DRT_PATH_BVH context host mode refuses a table whose tile rows hold a finite, nonzero direction with
 * | d.d - 1 | > 2^-42 (the message names the first such layer and pixel; nothing is changed, no film bit included); zero, NaN and
 * infinite directions are taken. Device mode cannot look at the table: there such rays are not held to the rule. Contexts scanned
 * out of LDS take any direction and give the rule's answer.
 */
typedef struct drt_ray_table
{
    const double *origins, *dirs, *weights; /* weights may be NULL */
    uint32_t      n_layers, flags;          /* flags: 0 or DRT_RAYS_DEVICE */
} drt_ray_table;                            /* 32 bytes */
int drt_bind_rays(drt_context *ctx, const drt_ray_table *t);   /* t == NULL: back to the camera */
/* Host pointers only: every device copies its own rows. All contexts are checked, and every device's copy is made, before any context
 * is changed: a call that fails on one device leaves the whole group as it was. */
int drt_group_bind_rays(drt_group *g, const drt_ray_table *t);

/*
 * Depth-cut films: beside the film of a render at max_depth D, the film the same render would leave at a shorter max_depth, for up
 * to DRT_MAX_DEPTH_CUTS depths at once and without tracing anything again. DESIGN.md section 5j.
 *
 * The rule: cut k of a context bound to depths d_0 < d_1 < ... holds, bit for bit, the film of a context created with
 * max_depth = d_k and otherwise the same parameters, after the same drt_render calls. The path generator is keyed by (seed, pixel,
 * sample) only, so that render walks the first d_k loop iterations of cast_ray (src/daily_ray_trace.c:440-472) of this one: its value
 * is `dst` after them, times the same vignette (:615), through the same film update (:732-743) with the sample's own number.
 *
 * A cut film has the main film's three buffers and layout: [tile_h*tile_w][S+1] sum + filter, [..][S] mean, [..][S] variance, owned
 * by the context, zero-filled at the bind and by drt_reset_film, released at the unbind and by drt_destroy. From the bind on every
 * sample drt_render adds to the film is added to every cut film too; a launch whose record pool ran out leaves them untouched and
 * is rendered again with the rest.
 */
#define DRT_MAX_DEPTH_CUTS 8
/* Bind the context to n cut depths (n == 0: unbind, the cut films are released). Refused, with the reason in drt_last_error() and the
 * context as it was: n > DRT_MAX_DEPTH_CUTS, a depth of 0 or above params.max_depth, depths not strictly ascending, DRT_MODE_XYZ, a
 * film that holds samples or an adaptive render (drt_reset_film first), an allocation failure. While cuts are bound
 * drt_render_adaptive and drt_render_adaptive_continue are refused. */
int drt_bind_depth_cuts(drt_context *ctx, const uint32_t *depths, uint32_t n);
/* Copy cut film `cut` (0 .. n-1) to host buffers (any may be NULL). Synchronises. */
int drt_read_depth_film(drt_context *ctx, uint32_t cut, double *pixels, double *avgs, double *vars);
/* Device pointers of cut film `cut`'s buffers; valid until the next bind, unbind or drt_destroy. */
int drt_depth_film_device_ptrs(drt_context *ctx, uint32_t cut, void **d_pixels, void **d_avgs, void **d_vars);
/* drt_read_xyz and drt_read_bgra of cut film `cut`: the same kernels over its buffers. Synchronise before they convert. */
int drt_read_depth_xyz(drt_context *ctx, uint32_t cut, double *xyz);
int drt_read_depth_bgra(drt_context *ctx, uint32_t cut, int which, uint8_t *bgra);
/* Every context is checked before any is changed; a device whose allocation fails leaves the whole group unbound. */
int drt_group_bind_depth_cuts(drt_group *g, const uint32_t *depths, uint32_t n);
/* Cut film `cut` of the whole tile, in image order, as drt_group_read_film. */
int drt_group_read_depth_film(drt_group *g, uint32_t cut, double *pixels, double *avgs, double *vars);

/*
 * Sensor films: beside the spectral film, the film some other sensor records -- up to DRT_MAX_SENSOR_CHANNELS channels, each the
 * sample's spectrum weighted by a caller-given curve and summed PER SAMPLE, so that every channel has a running mean and a variance
 * of its own (one path carries all wavelengths, so a channel's variance cannot be made from the film's per-wavelength variances).
 * DESIGN.md section 5l.
 *
 * The rule, for pixel p, sample number m (absolute: first_sample + s), the sample's contribution c[0..S) -- what the film update of
 * src/daily_ray_trace.c:732 takes, vignette included -- and the curves R[k][0..S); `+ - * /` only, nothing contracted:
 *   1. for each wavelength set j = 0 .. ceil(S/64) - 1: q[i] = R[k][64j+i] * c[64j+i] where 64j+i < S, and +0.0 elsewhere (i = 0..63);
 *   2. six times q = q[0::2] + q[1::2]; then t_j = q[0];
 *   3. v_k = t_0, then v_k = v_k + t_j for j = 1, 2, ... in order;
 *   4. v_k through the film update (:732-743): sum_k += v_k, the running mean and the variance accumulator with the divisor
 *      (double)(m + 1), the filter column += 1.0.
 *
 * The sensor film has the main film's three buffers with n channels where that has S wavelengths: [tile_h*tile_w][n+1] sum + filter,
 * [..][n] mean, [..][n] variance; owned by the context, zero-filled at the bind and by drt_reset_film, released at the unbind and by
 * drt_destroy. From the bind on every sample drt_render adds to the film is added to the sensor film too; a launch whose record pool
 * ran out leaves it untouched and is rendered again with the rest.
 */
#define DRT_MAX_SENSOR_CHANNELS 8
/* Bind the context to n curves of S values each (n == 0: unbind, the films are released). Refused, with the reason in
 * drt_last_error() and the context as it was: n > DRT_MAX_SENSOR_CHANNELS, null curves with n > 0, a curve value that is not finite,
 * DRT_MODE_XYZ, a film that holds samples, an adaptive render or a sample map (drt_reset_film first), bound depth cuts, an allocation
 * failure. While a sensor is bound drt_bind_depth_cuts, drt_render_adaptive, drt_render_adaptive_continue and drt_render_sample_map
 * are refused. */
int drt_bind_sensor(drt_context *ctx, const double *curves /* [n][S] */, uint32_t n);
/* Copy the sensor film to host buffers (any may be NULL). Synchronises. */
int drt_read_sensor_film(drt_context *ctx, double *pixels /* [P][n+1] */, double *avgs /* [P][n] */, double *vars /* [P][n] */);
/* Device pointers of the sensor film's buffers; valid until the next bind, unbind or drt_destroy. */
int drt_sensor_film_device_ptrs(drt_context *ctx, void **d_pixels, void **d_avgs, void **d_vars);
/* The sensor film as BMP pixel bytes. which: 0 = sum / filter, 1 = mean. Row r of the 3 x n matrix takes the channels to R, G, B
 * (m[r][0] * v_0, then + m[r][k] * v_k in order); then clamp to [0, 1], x 255, truncate (a NaN gives 0), stored B, G, R, 255.
 * Synchronises before it converts. */
int drt_read_sensor_bgra(drt_context *ctx, int which, const double *matrix /* [3][n] */, uint8_t *bgra);
/* Every context is checked, and every device's film allocated, before any context is changed. */
int drt_group_bind_sensor(drt_group *g, const double *curves, uint32_t n);
/* The sensor film of the whole tile, in image order, as drt_group_read_depth_film. */
int drt_group_read_sensor_film(drt_group *g, double *pixels, double *avgs, double *vars);

/*
 * Bucket films: the render's samples dealt out in turn to n films ("half buffers" at n = 2, the buckets of a median of means
 * otherwise), and a robust resolve over the n running means. The scatter of the n means estimates the error of their mean without
 * the film's own variance, and still does after a filter has been applied to each; the trimmed mean of the sorted means leaves
 * fireflies out. DESIGN.md section 5m.
 *
 * The rule, `+ - * /` and `<` only, nothing contracted. Sample number m (absolute: first_sample + s) belongs to bucket b = m % n as
 * that bucket's sample number j = m / n. Its contribution c[0..S) -- what the film update of src/daily_ray_trace.c:732 takes,
 * vignette included -- goes through the film update (:732-743) of bucket b's film only, with the divisor (double)(j + 1); that
 * film's filter column += 1.0. The samples of a bucket are applied in ascending m, also across several drt_render calls. With n = 1
 * the bucket film is the main film, bit for bit.
 *
 * The resolve, for trim count t, 0 <= 2 t < n, n >= 2, per pixel and wavelength over the buckets' running means x_0 .. x_{n-1}:
 *   1. mu = x_0, then mu = mu + x_b for b = 1 .. n-1 in order, then mu = mu / (double)n;
 *   2. d_b = x_b - mu; q = d_0 * d_0, then q = q + d_b * d_b in order; error = q / (double)(n * (n - 1)): the squared standard error
 *      of the mean across buckets, whatever t is;
 *   3. y = x sorted by odd-even transposition: for round r = 0 .. n-1, for i = r % 2, r % 2 + 2, ... < n - 1: when y[i+1] < y[i] the
 *      two change places. A comparison with a NaN is false, and so is -0 < +0: the network fixes where those end up;
 *   4. e = y[t], then e = e + y[i] for i = t+1 .. n-1-t in order; estimate = e / (double)(n - 2 t). t = 0: the mean in sorted order;
 *      t = (n-1)/2, n odd: the median; t = n/2 - 1, n even: the mean of the two middle values.
 *
 * Every bucket film has the main film's three buffers and layout: [tile_h*tile_w][S+1] sum + filter, [..][S] mean, [..][S] variance,
 * owned by the context, zero-filled at the bind and by drt_reset_film, released at the unbind and by drt_destroy. From the bind on
 * every sample drt_render adds to the film is added to its bucket's film too; a launch whose record pool ran out leaves them
 * untouched and is rendered again with the rest.
 */
#define DRT_MAX_BUCKETS 8
/* Bind the context to n buckets (n == 0: unbind, the films are released). Refused, with the reason in drt_last_error() and the
 * context as it was: n > DRT_MAX_BUCKETS, DRT_MODE_XYZ, a film that holds samples, an adaptive render or a sample map (drt_reset_film
 * first), bound depth cuts or a bound sensor, an allocation failure. While buckets are bound drt_bind_depth_cuts, drt_bind_sensor,
 * drt_render_adaptive, drt_render_adaptive_continue and drt_render_sample_map are refused. */
int drt_bind_buckets(drt_context *ctx, uint32_t n);
/* Copy bucket b's film (0 .. n-1) to host buffers (any may be NULL). Synchronises. */
int drt_read_bucket_film(drt_context *ctx, uint32_t b, double *pixels, double *avgs, double *vars);
/* Device pointers of bucket b's buffers; valid until the next bind, unbind or drt_destroy. Synchronises. */
int drt_bucket_film_device_ptrs(drt_context *ctx, uint32_t b, void **d_pixels, void **d_avgs, void **d_vars);
/* Run the resolve on the context's stream into two context-owned [P][S] buffers. Refused: nothing bound, n < 2, 2 * trim >= n, a
 * film of fewer than n samples (some bucket would be empty). */
int drt_resolve_buckets(drt_context *ctx, uint32_t trim);
/* The last resolve's results (either may be NULL), and their device addresses. Refused before any resolve, and after a render or a
 * reset that came later than the last resolve. */
int drt_read_bucket_resolve(drt_context *ctx, double *estimate /* [P][S] */, double *error /* [P][S] */);
int drt_bucket_resolve_device_ptrs(drt_context *ctx, void **d_estimate, void **d_error);
/* drt_read_xyz and drt_read_bgra's kernels with the estimate in the means' place (the picture is that of which = 1). */
int drt_read_bucket_resolve_xyz(drt_context *ctx, double *xyz);
int drt_read_bucket_resolve_bgra(drt_context *ctx, uint8_t *bgra);
/* Every context is checked, and every device's films allocated, before any context is changed. */
int drt_group_bind_buckets(drt_group *g, uint32_t n);
/* Bucket b's film of the whole tile, in image order, as drt_group_read_depth_film. */
int drt_group_read_bucket_film(drt_group *g, uint32_t b, double *pixels, double *avgs, double *vars);
/* Every context is checked before any resolves; the results of the whole tile, in image order. */
int drt_group_resolve_buckets(drt_group *g, uint32_t trim);
int drt_group_read_bucket_resolve(drt_group *g, double *estimate, double *error);

/*
 * Lobe films: the film split by what the first surface did with the light -- by the entry of vertex 0's own BDSF list whose addend
 * carries it, light sampled at vertex 0 (direct) and everything behind vertex 0 (indirect) apart -- and by emission the camera ray
 * itself ends on. These are the layers a compositor grades separately and a denoiser filters with different bandwidths. The film is
 * linear in the first vertex's BDSF addends (bdsf(), src/daily_ray_trace.c:215-229, and the light fold, :323-327, are linear per
 * addend), so the layers add up to the main film up to rounding. DESIGN.md section 5n.
 *
 * The rule, `+ - *` and the film update's `/` only, nothing contracted. For one sample, with f_i the i-th entry of vertex 0's list:
 *   - the addend a_i(args) is the value of the dispatcher's bdsf_result after entry i: the function's value, or, when its direction
 *     test fails, the value carried over from the entry before it (quirk Q1) -- 0.0 when nothing came before. It belongs to entry i's
 *     function even when it is a carried value: under this definition the films add up to the main film. On a reflected glass sample
 *     the reflectance film and the transmittance film both receive R, as the main film receives R + R;
 *   - R^c_K(args), for film c and map row K (direct or indirect): 0.0, then R = a_i + R over the positions i with K[f_i] == c, in
 *     list order;
 *   - C^c: 0.0, then for each visible light l in order C = C + R^c_direct(light l), C = C * em_l, C = C * c_l -- for every film;
 *   - vertex 0: dst^c = 0.0 + 1.0 * C^c and T^c = 1.0 * (R^c_indirect(sample) * dir_pdf);
 *   - vertex v >= 1: C_v and R_v are the main film's, shared by all films: dst^c = dst^c + T^c * C_v, T^c = T^c * (R_v * dir_pdf_v);
 *   - the end of the path, with n_shaded < max_depth and the path ending on an emitter: value^c = dst^c + T^c * spd(emitter) for every
 *     film when n_shaded >= 1; when n_shaded == 0, value = 0.0 + 1.0 * spd(emitter) for film `emission` and 0.0 for the others;
 *   - value^c * vignette goes through the film update (:732-743) of film c, the divisor the sample's own number + 1, the filter
 *     column += 1.0. Every film takes every sample, zeros included: each is a film of the main film's layout and count, and its
 *     variance is the layer's own.
 * A map that sends all 15 entries to film 0 gives the main film, bit for bit.
 *
 * Every lobe film has the main film's three buffers and layout, owned by the context, zero-filled at the bind and by drt_reset_film,
 * released at the unbind and by drt_destroy. A launch whose record pool ran out leaves them untouched and is rendered again with the
 * rest.
 */
#define DRT_MAX_LOBE_FILMS 8
#define DRT_LOBE_NONE 0xFFu            /* this part goes to no film */
typedef struct drt_lobe_map {
    uint8_t emission;                  /* a camera ray that ends on an emitter (no shaded vertex, term == 1) */
    uint8_t direct[DRT_NUM_BDSFS];     /* light sampled at vertex 0, by the listed function whose addend carries it */
    uint8_t indirect[DRT_NUM_BDSFS];   /* everything behind vertex 0, by the function whose addend carries the continuation */
    uint8_t pad_;
} drt_lobe_map;
/* Bind the context to n films and a map (n == 0: unbind, the films are released, the map is not read). Refused, with the reason in
 * drt_last_error() and the context as it was: n > DRT_MAX_LOBE_FILMS, a NULL map, a map entry >= n that is not DRT_LOBE_NONE,
 * DRT_MODE_XYZ, a film that holds samples, an adaptive render or a sample map (drt_reset_film first), bound depth cuts, a bound sensor
 * or bound buckets, an allocation failure. While lobes are bound drt_bind_depth_cuts, drt_bind_sensor, drt_bind_buckets,
 * drt_render_adaptive, drt_render_adaptive_continue and drt_render_sample_map are refused, and the live window is not used. */
int drt_bind_lobes(drt_context *ctx, uint32_t n, const drt_lobe_map *map);
/* Copy film c (0 .. n-1) to host buffers (any may be NULL). Synchronises. */
int drt_read_lobe_film(drt_context *ctx, uint32_t c, double *pixels, double *avgs, double *vars);
/* Device pointers of film c's buffers; valid until the next bind, unbind or drt_destroy. Synchronises. */
int drt_lobe_film_device_ptrs(drt_context *ctx, uint32_t c, void **d_pixels, void **d_avgs, void **d_vars);
/* drt_read_xyz and drt_read_bgra's kernels on film c (`which` as drt_read_bgra: 0 the sums, 1 the means, 2 the variances). */
int drt_read_lobe_xyz(drt_context *ctx, uint32_t c, double *xyz);
int drt_read_lobe_bgra(drt_context *ctx, uint32_t c, int which, uint8_t *bgra);
/* Every context is checked, and every device's films allocated, before any context is changed. */
int drt_group_bind_lobes(drt_group *g, uint32_t n, const drt_lobe_map *map);
/* Film c of the whole tile, in image order, as drt_group_read_depth_film. */
int drt_group_read_lobe_film(drt_group *g, uint32_t c, double *pixels, double *avgs, double *vars);

/*
 * Scene updates: move the camera and the surfaces of a live context, where the only way used to be drt_destroy + drt_create (the
 * pool freed and allocated again, the pool measurement rendered again, the hierarchy built again). DESIGN.md section 5g.
 *
 * The rule: after a successful call the context gives, for every later call -- drt_render, the adaptive calls, features, mattes, ray
 * queries, ray films, drt_read_* -- bit for bit the results of a fresh context that drt_create would make from the scene with surfaces
 * [first, first + count) replaced, or from the new camera, with the same drt_params, materials and spectral tables: films, hit logs, the
 * counting fields of drt_stats, RNG draw counts and query answers. Three things may differ from that fresh context, because none of them
 * can change a result bit: the shape of the hierarchy (it is refitted, not rebuilt, unless DRT_SURFACES_REBUILD asks), the size of the
 * record pool, and the shade kernel's dark-skip choice. The pool is NOT measured again: a launch that runs out of it is rendered again by
 * the existing mechanism, and drt_stats.redone_launches shows it.
 *
 * An update fixes the surface count and every surface's type and material (so the light list, the record width, the LDS layout and the
 * kernel instantiations stay); position, radius, normal, u and v may change on any surface, lights and point lights included.
 * History does not matter: the context keeps the caller's raw surfaces (a host copy from drt_create, a device copy made at the first
 * update), an update writes its range into that copy, and every table is derived again from all of it: update A then update B equals
 * update B alone. Both calls need a film without samples (a fresh context, or drt_reset_film), as drt_bind_rays does.
 *
 * Host mode (flags without DRT_SURFACES_DEVICE): everything is checked before anything changes, and the call is refused with a message
 * and nothing changed for: a null pointer with count > 0, first + count beyond the surface count, unknown flag bits; a film with samples;
 * a surface whose type or material differs from the one it replaces (the message names the first); and, in a DRT_PATH_BVH context,
 * coordinates that take the extent to 2^27 or beyond or (DRT_SURFACES_REBUILD) a tree deeper than the traversal stack -- drt_create's
 * two refusals. The caller's array is free when the call returns. count == 0 is a successful no-op (whatever the film holds). In a
 * context without the hierarchy DRT_SURFACES_REBUILD has nothing to build and changes nothing.
 *
 * Device mode: `surfaces` is count records of sizeof(drt_surface) (112 bytes) on the context's device; their type and material words are
 * not read. The work is enqueued on the context's stream and the call returns without waiting. The one condition the host cannot check
 * is the 2^27 extent: the kernel records a violation in a status word, and every later synchronising call (drt_synchronize, drt_read_*,
 * drt_get_stats) fails, naming it, until a later update or drt_set_camera brings the extent back. Renders enqueued in between are not
 * held to the rule but stay within their buffers (the box test only prunes). DRT_SURFACES_REBUILD with DRT_SURFACES_DEVICE is refused.
 *
 * drt_set_camera replaces the camera; in a DRT_PATH_BVH context the camera's reach is part of the extent, so the same derivation is
 * enqueued. It works while a ray table is bound (the film then does not depend on it).
 *
 * After either call results that describe the old scene are stale: drt_read_features / drt_read_mattes of a pass taken before it are
 * refused. Everything is rewritten in place on the context's stream, so what was enqueued before stays ordered before the update.
 */
#define DRT_SURFACES_DEVICE  1u /* `surfaces` is device memory on the context's device */
#define DRT_SURFACES_REBUILD 2u /* host mode only: build the hierarchy anew instead of refitting it */
int drt_set_camera(drt_context *ctx, const drt_camera *camera);
int drt_update_surfaces(drt_context *ctx, const drt_surface *surfaces, uint32_t first, uint32_t count, uint32_t flags);
/* Every context is checked, and every device's staging copy is made, before any context is changed. Host pointers only. Same bits for
 * any device list. */
/* drt_reset_film on every device: what a group needs between two frames, since both calls want a film without samples. */
int drt_group_reset_film(drt_group *g);
int drt_group_set_camera(drt_group *g, const drt_camera *camera);
int drt_group_update_surfaces(drt_group *g, const drt_surface *surfaces, uint32_t first, uint32_t count, uint32_t flags);
typedef struct drt_update_report
{
    uint32_t updates;            /* successful drt_update_surfaces (count > 0) and drt_set_camera calls */
    uint32_t refits_since_build; /* of those, the ones that refitted the hierarchy since it was last built (0 without DRT_PATH_BVH) */
    double   extent;             /* the extent the hierarchy's paddings are made for: max(camera reach, surfaces); 0 without DRT_PATH_BVH */
    double   kernel_ms;          /* HIP-event time of the last update's kernels (0: it launched none) */
} drt_update_report;             /* 24 bytes */
/* Waits for the last update's kernels. */
int drt_get_update_report(drt_context *ctx, drt_update_report *out);

/*
 * Material updates: new spectra and parameters for a live context -- a wall's colour, a light's spectrum or level, the glass's index,
 * the gold's n and k, a lobe's shininess or roughness -- where the only way used to be drt_destroy + drt_create. DESIGN.md section 5i.
 *
 * The rule is 5g's: after a successful call the context gives, for every later call -- drt_render, the adaptive calls, the denoiser,
 * features, mattes, ray queries, ray films, drt_read_* -- bit for bit the results of a fresh context that drt_create would make from the
 * scene with those SPD rows or material parameters replaced, with the same drt_params, surfaces and camera: films, hit logs, the counting
 * fields of drt_stats, RNG draw counts and query answers. The same three things may differ from that fresh context, because none can
 * change a result bit: the shape of the hierarchy, the size of the record pool, and the shade kernel's dark-skip choice. The pool is NOT
 * measured again, though a material edit can lengthen paths (an index of refraction, a roughness): a launch that runs out of it is
 * rendered again by the existing mechanism, and drt_stats.redone_launches shows it.
 *
 * History does not matter: the context keeps the caller's raw rows (a host copy from drt_create, a device copy made at the first
 * update), an update writes its range into that copy, and every derived table -- the diffuse / PI rows, the Fresnel pair rows, the
 * materials' two refract samples around 630 nm, the trace kernel's tail columns -- is made again from all of it: update A then update B
 * equals update B alone. Both calls need a film without samples (a fresh context, or drt_reset_film), as drt_update_surfaces does, and
 * both work under a bound ray table and in DRT_MODE_XYZ.
 *
 * drt_update_spectra gives rows [first_row, first_row + count) of the scene's SPD table (drt_scene.spds numbering) the values in
 * `rows`, [count][num_wavelengths] doubles. Any double is a legal value: the rule is whatever a fresh context makes of it, a NaN
 * included. The rows named by drt_scene.cmf_rw / cmf_x / cmf_y / cmf_z are the observer, not a material, and a range that holds one is
 * refused. Host mode (flags 0): the caller's array is free when the call returns. Device mode (DRT_SPECTRA_DEVICE): `rows` is memory on
 * the context's device; the work is enqueued on the context's stream and the call returns without waiting (the rows must stay until
 * the stream has passed it). There is nothing in it the host cannot check, so there is no status word.
 *
 * drt_update_materials takes whole drt_material records for materials [first, first + count) and accepts a difference in shininess and
 * roughness only: is_black_body, is_emissive, num_bdsfs, every bdsfs[j] below num_bdsfs, dir_func and all six SPD indices must equal
 * what the context holds (so the light list, the record width, the SPD table's layout and the kernel instantiations stay as drt_create
 * chose them; a material gets another colour by drt_update_spectra on its row). Host memory only; `flags` must be 0.
 *
 * Both calls check everything before anything changes and are refused, with a message and the context exactly as it was, for: a null
 * pointer with count > 0, a range beyond the table, unknown flag bits, a film with samples, a colour-matching row, a material field
 * other than the two (the message names the first material and field that differs). count == 0 is a successful no-op (whatever the
 * film holds). After either call results that describe the old scene are stale: drt_read_features / drt_read_mattes of a pass taken
 * before it are refused. Everything is rewritten in place on the context's stream, so what was enqueued before stays ordered before it.
 */
#define DRT_SPECTRA_DEVICE 1u /* `rows` is device memory on the context's device */
int drt_update_spectra(drt_context *ctx, const double *rows /* [count][S] */, uint32_t first_row, uint32_t count, uint32_t flags);
int drt_update_materials(drt_context *ctx, const drt_material *materials, uint32_t first, uint32_t count, uint32_t flags /* 0 */);
/* Every context is checked, and every device's staging copy is made, before any context is changed. Host pointers only. Same bits for
 * any device list. */
int drt_group_update_spectra(drt_group *g, const double *rows, uint32_t first_row, uint32_t count, uint32_t flags /* 0: host memory */);
int drt_group_update_materials(drt_group *g, const drt_material *materials, uint32_t first, uint32_t count, uint32_t flags /* 0 */);

/* Shape of the bounding-volume hierarchy drt_create() builds for scenes too large for LDS: node count, surfaces in
 * leaves, levels, and the traversal stack's capacity in entries (one per level at most; drt_create() refuses a deeper tree).
 * Host only: runs without a GPU. */
int drt_bvh_stats(const drt_scene *scene, uint32_t *nodes, uint32_t *leaf_surfaces, uint32_t *depth, uint32_t *stack_entries);

/* Arithmetic self-test kernels: evaluate op over n inputs on the device so tests can check
 * that f64 sqrt / divide / the path's sincos are bit-identical to the host. op: 0 sqrt(a),
 * 1 a/b, 2 sincos(a) -> out[2*i], out[2*i+1], 3 pow(a,b), 4 rng stream from key a (as u64 bits). */
int drt_selftest_arith(int device, int op, const double *a, const double *b, double *out, uint64_t n);

/* Path-id self-test: the trace kernel's decomposition of a path id into (launch pixel, sample in the launch) and of a tile pixel into
 * (i, j), run the way its refill runs it. Each of the n_draws waves starts at path id bases[w] (one 64-bit division, as at a draw
 * from the work counter) and hands out steps[0], steps[1], ... consecutive ids (each 1..64) by 32-bit arithmetic only. out holds four
 * words per id, draw after draw: id / n_samples, id % n_samples, and (id / n_samples) % tile_w, (id / n_samples) / tile_w. */
int drt_selftest_path_ids(int device, const uint64_t *bases, uint32_t n_draws, const uint32_t *steps, uint32_t n_steps, uint32_t n_samples,
                          uint32_t tile_w, uint64_t *out);

/* Device-function self-test: runs ONE of the path's device functions -- the very __device__ function the trace / shade
 * kernels call -- over n records (`in_stride` doubles in, `out_stride` doubles out per record), so that the edge cases of
 * the reference's functions (tangent / parallel / on-boundary rays, antiparallel rotation, disc centre, total internal
 * reflection) meet the HIP code directly and not only when a random scene happens to produce them. func:
 *   0 line_sphere_intersection  src/geometry.c:123-146   in o[3] d[3] c[3] r                 out t
 *   1 line_plane_intersection   src/geometry.c:157-182   in o[3] d[3] p[3] n[3] u[3] v[3]    out t
 *   2 vec3_reflect              src/geometry.c:85-90     in v[3] n[3]                        out r[3]
 *   3 vec3_transmit             src/geometry.c:92-106    in v[3] n[3] ir tr                  out t[3] (NaN on total internal reflection)
 *   4 find_rotation_between_vectors src/geometry.c:263-295  in v[3] w[3]                     out m[9], columns
 *   5 uniform_sample_sphere     src/rng.c:14-23          in rng state (u64 bits)             out p[3], state after (u64 bits)
 *   6 uniform_sample_disc       src/rng.c:25-51          in rng state (u64 bits)             out p[3], state after (u64 bits)
 *   7 ggx                       src/bdsf.c:3-20          in sn[3] mn[3] roughness            out D
 *   8 ggx_att                   src/bdsf.c:22-42         in v[3] sn[3] mn[3] roughness       out D * G1
 *   9 fs_dielectric_reflectance src/bdsf.c:44-67         in ir tr cos (one wavelength)       out R
 *  10 fs_conductor_reflectance  src/bdsf.c:78-101        in ir tr te cos (one wavelength)    out R
 *  11 seed_rng + rng            src/rng.c:1-12 (8a-R)    in path key (u64 bits)              out state (u64 bits), first rng()
 *  12 the hierarchy's f32 box test (prunes the scan of src/daily_ray_trace.c:340-364; no reference counterpart)
 *                                                          in o[3] d[3] lo[3] hi[3]            out lower bound of the entry distance, < 0: rejected
 *  13 line_plane_limited, the plane test of the LDS row scans (csrc/drt_device.h; the reference's function cut short where the scan's
 *     one comparison `t < limit` cannot come out true)    in func 1's 18, limit, want (0 = false)  out t where want and t < limit, else +inf
 *  14 the hierarchy's f32 sphere filter, sphere_certainly_missed (csrc/drt_kernels.h; spares the f64 intersector, no reference
 *     counterpart), on the leaf, the f32 ray and the f32 limit the walk makes from the record; E is the extent the leaf's pad is for
 *                                                          in o[3] d[3] c[3] r E limit         out 1 = "certainly missed" else 0, func 0's t */
int drt_selftest_unit(int device, int func, const double *in, uint32_t in_stride, double *out, uint32_t out_stride, uint64_t n);

/* Division self-test, records as in drt_selftest_unit: the forms that stand where the path loop had a `/` (csrc/drt_device.h,
 * csrc/drt_const_rule.h), beside that `/` on the same operands. Thread i of the launch runs record i, 64 consecutive records to a
 * wave: v_div_shared chooses per wave, so the caller decides by the order of the records which of them meet in one. func:
 *   0 v_div_shared        in v[3] f                 out v_div_shared(v, f)[3], v.x / f, v.y / f, v.z / f,
 *                                                       1 = the record's three scaled denominators are equal bit for bit (else 0),
 *                                                       1 = the record's wave shared the reciprocal (else 0: three plain divisions)
 *   1 drt_rng             in rng state (u64 bits)   out the draw, (state' >> 33) / 2147483647.0 by `/`, state' (u64 bits) */
int drt_selftest_division(int device, int func, const double *in, uint32_t in_stride, double *out, uint32_t out_stride, uint64_t n);

/* Material-layer self-test: runs n records (`in_stride` doubles in, `out_stride` doubles out per record) against the device scene of
 * ctx -- its materials, pair rows, diffuse * (1/PI) rows and refractive indices at trans_wl are the ones drt_create built -- through
 * the very __device__ functions the trace and shade kernels call, in their order. A record is a surface point:
 *     position[3] normal[3] out[3] on_dot  surface incident transmit          (13 doubles; material indices as whole numbers)
 * followed by, per func:
 *   0 evaluate: bdsf(), src/daily_ray_trace.c:215-229 with src/bdsf.c:105-186 -- eval_coefficients, record_media_word and fresnel_rows
 *     as the trace kernel writes a vertex, then bdsf_at_wavelength per wavelength on the table rows the shade kernel reads.
 *       in  +  bdsf  incoming[3]  mode                                         (18 doubles)
 *          bdsf: -1 the surface material's own list, or one DRT_BDSF_* id that replaces it (needs derived from that list; the pair
 *                rows are used only when the function is of the Fresnel kind they were tabulated for, else the record is unpaired)
 *          mode: bit 0 unpaired (PAIR_NONE: every Fresnel term from ir, tr, te), bit 1 the SIMPLE instantiation (no Fresnel cases)
 *       out reflectance[S], the EvalCoef flags word (bit 0 in == mirror direction, bit 1 in == refracted direction)   (S + 1)
 *   1 sample: sample_direction, src/bdsf.c:188-292
 *       in  +  dir_func  rng state (u64 bits)                                   (15 doubles)
 *          dir_func: -1 the surface material's own sampler, or a DRT_DIRF_* id
 *       out dir[3] recip_pdf, rng state after (u64 bits), rng draws taken      (6)
 * Returns nonzero (drt_last_error) and runs nothing when a record is narrower than its function needs, out_stride is too small, a
 * material index is not below num_materials, a bdsf / dir_func id is unknown (or the material's own dir_func is), or SIMPLE is asked of a
 * list that holds a Fresnel function. Synchronises. */
int drt_selftest_material(drt_context *ctx, int func, const double *in, uint32_t in_stride, double *out, uint32_t out_stride, uint64_t n);

/* Build-pass self-tests: two stages of a device hierarchy build (drt_rebuild_hierarchy below; csrc/drt_build_kernels.h) on arrays the
 * caller supplies, without a scene. Both go through the very enqueue helpers drt_rebuild_hierarchy goes through (the launch loops,
 * grids and buffer roles are the product's; only the buffers are scratch) on the null stream, and synchronise.
 *
 * drt_selftest_build_sort: the eight count / scan / scatter passes over m keys (1 <= m <= 2^24, every key below 2^63; the payload is
 * the position 0 .. m - 1, as the keys kernel writes it). keys_out[j] and pos_out[j] are the key and the position that end in slot j:
 * a stable sort, so pos_out is numpy's argsort(kind="stable"). Both halves of the sort's double buffer lie between guard words on the
 * device; the call fails (-3) if one of them changed. */
int drt_selftest_build_sort(int device, const uint64_t *keys, uint32_t m, uint64_t *keys_out, uint32_t *pos_out);
/* drt_selftest_build_topology: the status kernel and the level-by-level topology launches over m ascending keys (2 <= m <= 2^24; a
 * build launches nothing below 2), with nodes, leaves, leaf parents and leaf order of its own; tree_surf and pos are identities and
 * every surface is a sphere. child and count take the [m - 1][2] links of the nodes (csrc/drt_build_rule.h: step 6-7 of DESIGN.md
 * 5h), level_count the 33 level counts (inner nodes per depth, the root's 1 first), levels_out the level table: [m - 2] pairs
 * (inner node, parent * 2 + child slot), the deepest level first, in any order within a level. Keys out of order are refused. */
int drt_selftest_build_topology(int device, const uint64_t *sorted_keys, uint32_t m, int32_t *child, int32_t *count, uint32_t *level_count,
                                uint32_t *levels_out);
/* drt_selftest_live_resources: what this process holds through the library right now, over all contexts, groups and calls in flight:
 * out[0] device allocations, out[1] pinned host allocations, out[2] HIP events, out[3] HIP streams. Each goes up when one is made and
 * down when it is released, so a count that does not return to where it was after drt_destroy is a leak. Memory the caller bound with
 * drt_bind_film is the caller's and is not counted. Touches no device. */
int drt_selftest_live_resources(uint64_t out[4]);

/*
 * Device hierarchy builds: the tree of a live DRT_PATH_BVH context built anew on the device, from the context's own device copy of its
 * surfaces -- what a caller whose surfaces arrive in device memory (DRT_SURFACES_DEVICE) can do about a tree that refits have left the
 * wrong shape for (drt_update_report.refits_since_build), where DRT_SURFACES_REBUILD needs host surfaces and stops the stream.
 * DESIGN.md section 5h.
 *
 * drt_rebuild_hierarchy enqueues the work on the context's stream and returns without waiting for it: no stream synchronisation, no
 * blocking copy, and no allocation after the first call (drt_destroy frees the temporaries). What was enqueued before stays ordered
 * before it. The tree is a Morton-ordered one over the surfaces' current boxes, one surface per leaf, written into the allocations the
 * context has; its shape is a deterministic function of the boxes (csrc/drt_build_rule.h, restated in tests/hierarchy_rule.py) and it
 * is never deeper than the traversal stack, by construction.
 *
 * No result changes: the hierarchy only prunes, so films, hit logs, the counting statistics and RNG draw counts are bit for bit what
 * they were. The call needs no empty film and may come between two drt_render calls of one film. It is not an update:
 * drt_update_report.updates does not move, refits_since_build goes to 0, features and mattes that have been read stay readable, and a
 * pending 2^27 extent violation of a device-mode update stays pending. In a context without the hierarchy the call returns 0 and
 * changes nothing. `flags` must be 0. Refits (drt_update_surfaces, drt_set_camera), DRT_SURFACES_REBUILD and further device builds
 * work afterwards in any order; the first of them, or drt_read_hierarchy, waits for the host's copy of the tree's links to arrive.
 */
int drt_rebuild_hierarchy(drt_context *ctx, uint32_t flags);
/* Every context from its own device copy. Same bits for any device list. */
int drt_group_rebuild_hierarchy(drt_group *g, uint32_t flags);
typedef struct drt_hierarchy_report
{
    uint32_t nodes, leaf_surfaces; /* BvhNode records and leaf slots (0, 0 without DRT_PATH_BVH) */
    uint32_t depth;                /* levels, as drt_bvh_stats counts them */
    uint32_t device_builds;        /* successful drt_rebuild_hierarchy calls that built a tree */
    uint32_t built_by;             /* who made the tree in use: 0 the host (drt_create, DRT_SURFACES_REBUILD), 1 the device */
    uint32_t pad;
    double   kernel_ms;            /* HIP-event time of the last device build's kernels (0: there was none) */
} drt_hierarchy_report;            /* 32 bytes */
/* Waits for the last device build. */
int drt_get_hierarchy_report(drt_context *ctx, drt_hierarchy_report *out);
/* The tree in use: `nodes` takes n_nodes records of 64 bytes (csrc/drt_kernels.h, BvhNode: float lo[2][3], hi[2][3]; int32 child[2],
 * count[2]), leaf_surface the surface index of every leaf slot. n_nodes and n_leaf must be the report's counts. Synchronises. */
int drt_read_hierarchy(drt_context *ctx, void *nodes, uint32_t n_nodes, uint32_t *leaf_surface, uint32_t n_leaf);

/*
 * The live window: the rectangle of image pixels [x_lo, x_hi) x [y_lo, y_hi), clipped to the tile, outside which no camera ray can
 * reach the scene, whatever the pixel draws (csrc/drt_window_rule.h; DESIGN.md section 3 has the proof). out = {x_lo, x_hi, y_lo,
 * y_hi}; x_lo == x_hi: empty, the scene is wholly off the tile. It is the whole tile -- {x0, x0 + tile_w, y0, the tile's last image
 * row + 1} -- where the rule does not apply: a lens camera (aperture_radius > 0), an escape material that emits or is no black body,
 * a scene corner not in front of the pinhole, a coordinate that is not finite.
 * Dense renders (drt_render, drt_render_tile, the group forms) trace and shade the window's pixels only; every other tile pixel gets,
 * per kernel pair, what its samples -- all worth +0 -- leave on the film, and its paths are counted in drt_stats as the reference
 * counts them (a path, one closest-hit scan, the pixel's draws). Films, statistics and draw counts are bit for bit what they are
 * without it; DRT_NO_LIVE_WINDOW=1, read by drt_create, turns it off. Not used with DRT_FLAG_RECORD_HITS, pixel lists (adaptive
 * rounds, sample maps), a bound ray table, bound depth cuts, a bound sensor, bound buckets or bound lobes.
 */
/* Host only, like drt_bvh_stats: the rule on the scene and camera as given. */
int drt_live_window_of(const drt_scene *scene, const drt_camera *camera, const drt_params *params, uint32_t out[4]);
/* The live context's: follows drt_set_camera, host-mode drt_update_surfaces and hierarchy rebuilds; after a device-mode surface update
 * the host does not know the scene's bounds, and the window is the whole tile until a host-mode update. */
int drt_live_window(drt_context *ctx, uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* DRT_HIP_H */
