/*
 * drt_launcher.hip -- the C-ABI of include/drt_hip.h: scene upload (AoS boundary structs -> SoA
 * device tables), film ownership, batch scheduling of the trace and shade kernels on one HIP
 * stream, HIP-event timing, statistics. gfx950 only; there is no CPU path in this library.
 */
#include "drt_kernels.h"
#include "drt_bvh_kernels.h"
#include "drt_adaptive_kernels.h"
#include "drt_sample_map_kernels.h"
#include "drt_denoise_kernels.h"
#include "drt_feature_kernels.h"
#include "drt_matte_kernels.h"
#include "drt_ray_kernels.h"
#include "drt_update_kernels.h"
#include "drt_build_kernels.h"
#include "drt_material_kernels.h"
#include "drt_depth_kernels.h"
#include "drt_sensor_kernels.h"
#include "drt_bucket_kernels.h"
#include "drt_lobe_kernels.h"
#include "drt_window_kernels.h"
#include "drt_window_rule.h"
#include "drt_pair_rule.h"
#include "drt_shade_lds_rule.h"
#include "drt_owned.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <chrono>
#include <vector>

static thread_local std::string g_last_error;

#define RAY_STAGING_RAYS (1u << 20) /* host-mode ray queries go through device buffers of this many rays, chunk by chunk */
#define DRT_DEFAULT_MAX_BATCH 256 /* samples per kernel pair when the caller leaves batch_spp = 0 */

/* d_counters, in 8-byte words: [0, DRT_NUM_COUNTERS) the statistics of complete kernel pairs; then the WORK words of the pair in
 * flight -- +0 trace queue, +1 shade queue, +2 bounce queue length, +3 spare, +4 pool cursor (zeroed before every trace launch),
 * +5 overflow flag, +6 sequence number of the last complete pair, +7 peak of the pool cursor -- then, at DRT_PAIR_COUNTERS, the
 * statistics of the pair in flight: the kernels count there, and drt_mark_pair_kernel adds them to the totals only when the pair
 * was complete (a pair whose pool ran out is rendered again, and would be counted twice) */
#define DRT_PAIR_COUNTERS (DRT_NUM_COUNTERS + 8)
#define DRT_COUNTER_WORDS (DRT_PAIR_COUNTERS + DRT_NUM_COUNTERS)

static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                      \
    do                                                                                                     \
    {                                                                                                      \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return fail(-100 - (int)e_, "%s: %s", #expr, hipGetErrorString(e_));         \
    } while (0)

/* the two memory policies of Owned (drt_owned.h), each with its count of live allocations */
struct DeviceMem
{
    static std::atomic<uint64_t> &live() { static std::atomic<uint64_t> n{0}; return n; }
    static hipError_t alloc(void **p, size_t bytes)
    {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) live() += 1;
        return e;
    }
    static void free(void *p) { (void)hipFree(p); live() -= 1; }
};
struct PinnedMem
{
    static std::atomic<uint64_t> &live() { static std::atomic<uint64_t> n{0}; return n; }
    static hipError_t alloc(void **p, size_t bytes)
    {
        const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) live() += 1;
        return e;
    }
    static void free(void *p) { (void)hipHostFree(p); live() -= 1; }
};
template <typename T> using DevBuf = Owned<T, DeviceMem>;
template <typename T> using PinnedBuf = Owned<T, PinnedMem>;

struct drt_context
{
    int         device = 0;
    hipStream_t stream = nullptr;
    Stream      own_stream; /* declared before every buffer and event: destroyed after all of them */
    drt_params  params{};
    DevScene    dsc{};
    DevCamera   dcam{};
    uint32_t    cmf_rw = 0, cmf_x = 0, cmf_y = 0, cmf_z = 0;
    double      interval = 0.0;

    std::vector<DevBuf<unsigned char>> allocations; /* scene tables */
    std::vector<DevMaterial> host_mats;        /* what d.mats holds (drt_selftest_material derives its override tables from it) */
    DevMaterial *d_mat_variants = nullptr;     /* (held by `allocations`) those tables, made on the first drt_selftest_material call */
    double *d_pixels = nullptr, *d_avgs = nullptr, *d_vars = nullptr; /* XYZ film mode: d_pixels is [n_pix][XYZ_FILM_WORDS], the others stay null */
    DevBuf<double> own_pixels, own_avgs, own_vars; /* own_film: what the three point at; after drt_bind_film they point at the caller's memory, never freed here */
    bool    xyz_mode = false;
    bool    own_film = false;
    DevBuf<uint64_t> d_records, d_headers;
    uint32_t  light0_em_spd = 0;      /* emission SPD row of the first light (0 when there is none) */
    DevBuf<double> d_tail_stage; /* [n_pix * batch][tail_count]: per-sample results of the shade kernel's tail pass */
    DevBuf<double> d_tail_resume; /* [n_pix * batch][tail_count]: the throughput the trace kernel carried for a path it handed over at a vertex
                                          k >= 1 (TraceParams::tail_resume); only where trace_tail && !tail_all_staged && tail_resume */
    uint32_t  batch_spp = 1;
    uint32_t  vertex_words = 0, vertex_shift = 0, block_words = 0; /* a vertex record, its log2, a pool block (four vertices), in 8-byte words */
    uint64_t  pool_blocks = 0;          /* blocks in d_records */
    uint32_t  worst_blocks_per_path = 0; /* what a path of max_depth vertices takes (table block included) */
    double    est_blocks_per_path = 0.0; /* measured on a sample of the tile when the context is created */
    struct Batch { PairSpan span; uint64_t seq; }; /* (drt_pair_rule.h) */
    std::vector<Batch> inflight;         /* kernel pairs enqueued since the last synchronisation (redone if the pool ran out) */
    uint64_t  next_seq = 1;
    uint64_t  redone_batches = 0, pool_peak = 0;
    DevBuf<int32_t> d_hits;
    uint64_t  hits_capacity = 0; /* in paths */
    uint32_t  hits_samples = 0;
    DevBuf<unsigned long long> d_counters; /* DRT_COUNTER_WORDS words: layout at DRT_PAIR_COUNTERS above */
    DevBuf<PrimaryHit> d_primary;         /* BVH pipeline: closest hit of every path's camera ray (drt_bvh_kernels.h) */
    DevBuf<uint64_t> d_queue;         /* BVH pipeline: ids of the paths that go on after their first hit */
    bool        bvh_pipeline = false;
    int         primary_grid_cap = 0, bounce_grid_cap = 0;
    DevBuf<double> d_xyz;
    DevBuf<uint8_t> d_bgra;
    bool      trace_tail = false;     /* the trace kernel carries the tail wavelengths of the paths it can (drt_trace_kernel<true, true>): those of plastic
                                         and mirror vertices only, and those without a vertex */
    bool      tail_all_staged = false; /* ... and in this scene that is every path: the shade kernel's tail pass has nothing to replay */
    bool      tail_resume = false;     /* ... and where it is not, the tail pass resumes a path from the vertex the trace kernel carried it to (DRT_TAIL_RESUME=0: off) */
    bool      dark_skip = true;        /* the shade kernel's instantiation that passes over samples worth 0 in pixels nothing has reached yet: for
                                          pairs over the whole tile or a pixel list, from the TILE's vertices per path */
    bool      dark_skip_win = true;    /* ... and for windowed pairs, from the live window's own (shade_dark()) */
    bool      no_fixed_lists = false;  /* DRT_NO_FIXED_LISTS, read when the context is created: the shade kernel's fixed-list bodies are not taken */
    bool      simple_bdsfs = false;    /* no material lists anything but bp_diffuse_bdsf, bp_glossy_bdsf, mirror_bdsf: the shade kernel without the Fresnel code */
    bool      no_closed_shade = false; /* DRT_NO_CLOSED_SHADE, read when the context is created: the closed shade instantiation is not taken */
    bool      closed_lists = false;    /* every material lists nothing, or exactly one of the lists with straight-line code (closed_lists()): the
                                          shade kernel without the general list. Decided with simple_bdsfs; a material update keeps every list
                                          (materials_check), so no later call can change it */
    const double *d_spd_tail = nullptr; /* (held by `allocations`) [n_spd][tail_count]: the SPD table's tail columns */

    bool   scene_in_lds = true, spds_in_lds = true, use_bvh = false;
    size_t trace_lds = 0, shade_lds = 0;
    size_t shade_lds_closed = 0; /* dynamic LDS of drt_shade_kernel_closed_lds, whose waves have a region of their own size (shade_lds: every other shade kernel) */
    bool   closed_lds = false;   /* a closed context launches drt_shade_kernel_closed_lds: five of its workgroups fit a compute unit's LDS, and DRT_NO_CLOSED_LDS was not set when the context was created */
    bool trace_stash = false; /* camera launches run the stash form, drt_trace_kernel, with TRACE_STASH_BYTES of LDS behind trace_lds; else drt_trace_direct_kernel */
    size_t shade_lds_closed6 = 0; /* dynamic LDS of drt_shade_kernel_closed_lds6: one table and eight wave regions */
    bool   closed_lds6 = false;   /* a closed context's dense launches run drt_shade_kernel_closed_lds6, six waves per SIMD: the occupancy query gave three of its 512-lane
                                     workgroups per compute unit, and DRT_CLOSED_WAVES did not ask for fewer when the context was created */
    int    shade_grid_cap6 = 0;   /* ... and their persistent grid (shade_grid_cap: every other shade launch, the context's adaptive rounds among them) */
    int    trace_grid_cap = 0, shade_grid_cap = 0;
    uint32_t trace_chunk_override = 0; /* DRT_TRACE_CHUNK tuning knob */
    ShadeOverrides shade_overrides;    /* DRT_SHADE_CHUNK, DRT_SHADE_SUBS, DRT_TAIL_PERIOD tuning knobs (drt_pair_rule.h) */
    uint32_t debug_shade_mode = 0;     /* DRT_DEBUG_SHADE_MODE timing probe: 1 main pass only, 2 tail pass only */
    bool     debug_tail_phase_a_off = false; /* DRT_DEBUG_TAIL_PHASE_A_OFF timing probe: the tail pass is left its film update only */
    uint32_t shade_sets = 1, tail_first = 0, tail_count = 0;
    uint64_t n_pix = 0;

    std::vector<Event> ev; /* triples: trace start, trace end / shade start, shade end */
    std::vector<double> ev_paths; /* per triple: the paths of that kernel pair */
    size_t ev_used = 0;
    double trace_ms = 0.0, shade_ms = 0.0;
    uint64_t timed_pairs = 0; /* per sample pass over the tile (src/daily_ray_trace.c:746-756): min, max, running mean over the pairs */
    double min_sample_ms = 0.0, max_sample_ms = 0.0, avg_sample_ms = 0.0;

    /* adaptive sampling (drt_render_adaptive): the film has had samples from drt_render / drt_write_film, or an adaptive render */
    bool film_used = false, adaptive_done = false;
    DevBuf<uint32_t> d_counts;        /* [n_pix] samples per pixel */
    DevBuf<uint32_t> d_alist[2]; /* the round's active pixels and the next round's (ping-pong) */
    DevBuf<unsigned long long> d_keep; /* [ceil(n_pix / 64)] keep bits */
    DevBuf<uint32_t> d_bkeep;         /* [blocks of drt_converge_kernel + 1]: per block, then the active count */
    DevBuf<uint32_t> d_ainfo;         /* [1 + ADOPT_WORDS]: pixels at max_spp so far, then the report of the adoption kernels */
    PinnedBuf<uint32_t> h_active;         /* pinned host words the active count, then d_ainfo, are copied to: the copies stay asynchronous,
                                              so the devices of a group are all given their round before any is waited for */
    /* n: the count all active pixels hold (same); !same: they hold different counts, each max_spp - count a multiple of step */
    /* the denoiser (drt_denoise_film): its result and work buffers, kept from call to call, and the film they were made from */
    uint64_t film_gen = 0;                 /* counts what changes the film: kernel pairs, drt_write_film, drt_reset_film, drt_bind_film */
    uint64_t dn_gen = 0;                   /* film_gen at the last drt_denoise_film */
    bool     dn_valid = false;
    DevBuf<double> d_dn_mean, d_dn_var, d_dn_guide, d_dn_weights, d_dn_wsum;
    DevBuf<uint32_t> d_dn_unusable;
    uint32_t dn_window_cap = 0;            /* window entries per pixel d_dn_weights holds */
    /* first-hit features (drt_render_features): what the colour table is made from, the result, and the film it took its counts from */
    std::vector<drt_material> ft_mats;     /* the scene's materials and SPD rows as the caller gave them */
    std::vector<double> ft_spds;
    uint32_t ft_n_spd = 0, ft_S = 0;
    DevBuf<double> d_ft_mean, d_ft_m2, d_ft_colour;
    DevBuf<int32_t> d_ft_ids;
    DevBuf<uint32_t> d_ft_counts, d_ft_report;
    DevBuf<unsigned long long> d_ft_info;
    Event    ft_ev[2];
    bool     ft_valid = false, ft_from_film = false;
    uint64_t ft_gen = 0;                   /* film_gen at the last drt_render_features */
    /* ID mattes (drt_render_mattes): the result and the film it took its counts from; d_ft_counts and d_ft_report are shared */
    DevBuf<int32_t> d_mt_ids, d_mt_list;
    DevBuf<uint32_t> d_mt_counts, d_mt_tail;
    DevBuf<double> d_mt_cover;
    DevBuf<unsigned long long> d_mt_info;
    Event    mt_ev[2];
    bool     mt_valid = false, mt_from_film = false;
    uint64_t mt_gen = 0;                   /* film_gen at the last drt_render_mattes */
    /* ray queries (drt_cast_rays, drt_test_visibility, drt_cast_pixels): the staging buffers of host mode, made when first needed */
    uint64_t ray_chunk = RAY_STAGING_RAYS; /* rays per host-mode launch (DRT_RAY_CHUNK: a test knob, read here at creation) */
    int      ray_grid_cap = 1;
    DevBuf<double> d_ray_a, d_ray_b;
    DevBuf<drt_ray_hit> d_ray_hits;
    DevBuf<uint8_t> d_ray_visible;
    DevBuf<uint32_t> d_ray_xy, d_ray_samples;
    /* ray films (drt_bind_rays): the table the ray-mode kernels read, and the device copies of the tile's rows that host mode made */
    bool        rays_bound = false;
    DevRayTable rt{};
    DevBuf<double> d_rt_origins, d_rt_dirs, d_rt_weights;
    /* scene updates (drt_update_surfaces, drt_set_camera; drt_update_kernels.h): the caller's raw surfaces on both sides, the host's
     * tree, and what the three kernels read. Everything on the device is made at the first update. */
    std::vector<drt_surface> h_surfaces;   /* as drt_create got them, with every host-mode update written in */
    bool      h_stale = false;             /* a device-mode update has gone into d_raw only: read it back before the host decides anything */
    std::vector<BvhNode>  h_nodes;         /* hierarchy contexts: the tree's links (its boxes are the device's business after an update) */
    std::vector<uint32_t> h_order;         /* ... and the surface in every leaf slot */
    double    cam_reach = 0.0, extent = 0.0; /* the camera's share of the extent; the extent in use (hierarchy contexts) */
    bool      extent_known = true;
    bool      upd_ready = false;
    DevBuf<drt_surface> d_raw; PinnedBuf<drt_surface> h_stage; /* the device copy; the pinned buffer host mode goes through */
    DevBuf<int32_t> d_light_slot;
    DevBuf<double> d_boxes;
    DevBuf<uint32_t> d_leaf_parent;
    DevBuf<uint2> d_levels;
    std::vector<uint32_t> level_first;     /* level l, deepest first, is d_levels[level_first[l] .. level_first[l + 1]) */
    DevBuf<unsigned long long> d_upd_status;
    Event     upd_ev[3]; /* the last update's kernels: start, end; the pinned buffer is free again */
    bool      upd_timed = false, stage_busy = false;
    bool      upd_check = false, upd_violation = false; /* device mode: the status word is to be read at the next synchronisation; what it said */
    uint32_t  updates = 0, refits = 0;
    double    upd_ms = 0.0;
    /* device hierarchy builds (drt_rebuild_hierarchy; drt_build_kernels.h): the temporaries, made at the first one, and the host's
     * copy of the tree on its way back */
    bool      boxes_valid = false;         /* d_boxes and the extent word hold the current surfaces' (an update has run the derive kernel) */
    bool      hb_ready = false, hb_timed = false;
    bool      hb_mirror_pending = false;   /* h_nodes, h_order and level_first are the tree before the last device build: hb_ev[2] says when hb_mirror holds the new ones */
    DevBuf<uint32_t> d_hb_tree_surf, d_hb_pos[2], d_hb_table, d_hb_order;
    DevBuf<uint64_t> d_hb_keys[2];
    DevBuf<uint4> d_hb_items[2];
    DevBuf<unsigned char> d_hb_status; PinnedBuf<unsigned char> hb_mirror; /* BUILD_STATUS_BYTES; pinned: nodes, leaf order, level counts */
    Event     hb_ev[3]; /* the last build's kernels: start, end; its copy into hb_mirror */
    uint32_t  hb_builds = 0, hb_built_by = 0, hb_depth = 0;
    double    hb_ms = 0.0;
    /* material updates (drt_update_spectra, drt_update_materials; drt_material_kernels.h): how every row of d.spds is made (recorded by
     * build_device_scene), the caller's raw rows on the device, and the pinned buffers host mode goes through. Everything on the device
     * is made at the first update. */
    std::vector<SpdRowDesc> spd_desc;      /* [d.n_spd] */
    bool      mu_ready = false;
    bool      spd_stale = false;           /* a device-mode update has gone into d_spd_raw only: ft_spds and host_mats' refract_i0 / refract_i1 are read back before the host uses them */
    bool      variants_stale = false;      /* d_mat_variants was made from host_mats as they were before an update */
    DevBuf<SpdRowDesc> d_spd_desc;
    DevBuf<double> d_spd_raw, d_spd_in; PinnedBuf<double> h_spd_stage; /* [ft_n_spd][S] each: raw rows; host mode's rows on the device; pinned */
    DevBuf<int32_t> d_mat_refract;    /* [n_mat] */
    PinnedBuf<DevMaterial> h_mat_stage;    /* pinned, [n_mat] */
    Event     mu_ev[2]; /* the copies out of h_spd_stage and h_mat_stage are done */
    bool      spd_stage_busy = false, mat_stage_busy = false;
    uint32_t  spectra_updates = 0, material_updates = 0;
    /* depth cuts (drt_bind_depth_cuts; drt_depth_kernels.h): the bound depths, ascending, and one film per cut, laid out as the main film */
    uint32_t  n_cuts = 0, cut_depth[DRT_MAX_DEPTH_CUTS] = {};
    struct CutFilms { DevBuf<double> pixels[DRT_MAX_DEPTH_CUTS], avgs[DRT_MAX_DEPTH_CUTS], vars[DRT_MAX_DEPTH_CUTS]; } cuts;
    int       depth_grid_cap = 1;
    /* sensor film (drt_bind_sensor; drt_sensor_kernels.h): n curves of S values, and one film of n channels laid out as the main film */
    uint32_t  n_sensor = 0;
    struct SensorFilm { DevBuf<double> curves, pixels, avgs, vars; bool spds_in_lds = false; int grid_cap = 1; } sensor;
    /* bucket films (drt_bind_buckets; drt_bucket_kernels.h): one film per bucket, laid out as the main film; the samples drt_render has
     * added since the bind or the last reset (only uniform renders are allowed while bound, so one count holds for every pixel); the
     * resolve's two [n_pix][S] results, the film they were made from, and the estimate with a filter column of 1 for drt_film_xyz_kernel */
    uint32_t  n_buckets = 0;
    struct BucketFilms { DevBuf<double> pixels[DRT_MAX_BUCKETS], avgs[DRT_MAX_BUCKETS], vars[DRT_MAX_BUCKETS]; int grid_cap = 1; } buckets;
    uint64_t  bk_samples = 0;
    DevBuf<double> d_bk_estimate, d_bk_error, d_bk_packed;
    bool      bk_valid = false;
    uint64_t  bk_gen = 0;                  /* film_gen at the last drt_resolve_buckets */
    /* lobe films (drt_bind_lobes; drt_lobe_kernels.h): one film per lobe film, laid out as the main film, and the map that routes them */
    uint32_t  n_lobes = 0;
    drt_lobe_map lobe_map{};
    struct LobeFilms { DevBuf<double> pixels[DRT_MAX_LOBE_FILMS], avgs[DRT_MAX_LOBE_FILMS], vars[DRT_MAX_LOBE_FILMS]; int grid_cap = 1; } lobes;
    /* sample maps (drt_render_sample_map; drt_sample_map_kernels.h): the call's remainders, host targets on their way to the adopt
     * kernel, the report and its pinned copy -- a set of its own, whole or absent like the adaptive one it is used with */
    DevBuf<uint32_t> d_sm_rem, d_sm_targets, d_sm_report;
    PinnedBuf<uint32_t> h_sm_report;
    uint32_t  sm_bits = 0;                 /* the rounds of the call in progress that are still to be enqueued: bits of this device's B */
    struct Adaptive { drt_adaptive a; uint32_t n = 0, n_in = 0, k = 0, active = 0; int cur = 0; bool first = true, same = true; uint64_t redone = 0; } ad;
    /* the live window (drt_window_rule.h, drt_window_kernels.h): dense pairs trace and shade its pixels only, on a compact staging film */
    drt_camera h_camera{};                 /* the camera as the caller gave it (drt_create, drt_set_camera) */
    bool      win_allowed = true;          /* not DRT_NO_LIVE_WINDOW, read when the context is created */
    bool      win_dirty = true;            /* camera, surfaces or hierarchy have changed since `win` was worked out */
    LiveWindow win{};                      /* in image pixels; whole: the rule does not apply */
    uint32_t  wx0 = 0, wx1 = 0, wy0 = 0, wy1 = 0; /* ... and in tile columns and tile rows */
    bool      win_part = false;            /* the window is a proper part of the tile (possibly empty): what a dense pair can use */
    bool      win_open = false;            /* between window_open and window_close: the pairs in between are windowed ones */
    DevBuf<double> d_win_film[3];          /* the staging film [win rows][win columns], laid out as the film */
    uint64_t  win_film_pix = 0;            /* pixels it holds */
};

static size_t trace_lds_bytes(uint32_t n_surf, uint32_t n_lights, uint32_t n_mat)
{
    size_t b = TRACE_CONST_BYTES; /* the launch constants, in front (DRT_TRACE_CONST == 1 only) */
    b += (size_t)(SR_STRIDE + SF_COUNT) * n_surf * 8 + (size_t)LF_COUNT * n_lights * 8;
    b += ((size_t)(2 * n_surf + 2 * n_lights) * 4 + 7) & ~(size_t)7;
    b += (size_t)n_mat * sizeof(DevMaterial);
    b += (size_t)(TRACE_BLOCK / 64) * TRACE_LANE_ROWS * 64 * 8; /* the waves' lane rows (TRACE_LW_*) */
    return b;
}

template <typename T>
static int upload(drt_context *ctx, const std::vector<T> &host, const T **dev)
{
    DevBuf<unsigned char> buf;
    HIP_TRY(buf.need(std::max<size_t>(host.size(), 1) * sizeof(T)));
    unsigned char *p = buf;
    ctx->allocations.push_back(std::move(buf));
    if (!host.empty()) HIP_TRY(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    *dev = (const T *)p;
    return 0;
}

static V3 hv(const double a[3]) { V3 r; r.x = a[0]; r.y = a[1]; r.z = a[2]; return r; }

/* host-side twins of the device vector ops used for per-surface constants (same IEEE ops) */
static double h_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static double h_length(const double a[3]) { return std::sqrt(h_dot(a, a)); }

/* ---- BVH over the surfaces of a large scene (host build: median split, padded boxes) ---- */
struct BuildPrim
{
    double   lo[3], hi[3], c[3];
    uint32_t idx;
};

/* Box of everything a surface's intersector can report a hit on. A plane accepts the points j (relative to its
 * `position`) of the plane through it with 0 <= j.u^ <= |u| and 0 <= j.v^ <= |v| (src/geometry.c:157-182): the rectangle
 * position + a u + b v only when u and v are perpendicular; for slanted edge vectors it is the parallelogram whose
 * corners solve [u^; v^; n] j = (a, b, 0) at the four (a, b) extremes -- bounded here by solving exactly that. */
static void prim_bounds(const drt_surface &s, double lo[3], double hi[3])
{
    if (s.type == DRT_GEO_SPHERE)
    {
        for (int k = 0; k < 3; k += 1)
        {
            lo[k] = s.position[k] - std::fabs(s.radius);
            hi[k] = s.position[k] + std::fabs(s.radius);
        }
    }
    else
    {
        const double ul = h_length(s.u), vl = h_length(s.v);
        const double un[3] = {s.u[0] / ul, s.u[1] / ul, s.u[2] / ul}, vn[3] = {s.v[0] / vl, s.v[1] / vl, s.v[2] / vl};
        const double *n = s.normal;
        /* rows of M = u^, v^, n; its inverse by cofactors */
        const double c0[3] = {vn[1] * n[2] - vn[2] * n[1], vn[2] * n[0] - vn[0] * n[2], vn[0] * n[1] - vn[1] * n[0]}; /* v^ x n */
        const double c1[3] = {n[1] * un[2] - n[2] * un[1], n[2] * un[0] - n[0] * un[2], n[0] * un[1] - n[1] * un[0]}; /* n x u^ */
        const double det = un[0] * c0[0] + un[1] * c0[1] + un[2] * c0[2];
        const bool ok = std::isfinite(det) && std::fabs(det) > 1e-6 && std::isfinite(ul) && std::isfinite(vl);
        for (int k = 0; k < 3; k += 1)
        {
            lo[k] = HUGE_VAL;
            hi[k] = -HUGE_VAL;
        }
        for (int corner = 0; corner < 4 && ok; corner += 1)
        {
            const double a = (corner & 1) ? ul : 0.0, b = (corner & 2) ? vl : 0.0;
            for (int k = 0; k < 3; k += 1)
            {
                double j = (a * c0[k] + b * c1[k]) / det; /* M^-1 (a, b, 0) */
                lo[k] = std::min(lo[k], s.position[k] + j);
                hi[k] = std::max(hi[k], s.position[k] + j);
            }
        }
        if (!ok) /* edge vectors (nearly) parallel, or a normal in their span: the accepted region is unbounded */
            for (int k = 0; k < 3; k += 1)
            {
                lo[k] = -1e300;
                hi[k] = 1e300;
            }
    }
    for (int k = 0; k < 3; k += 1)
    {
        /* pad: a hit the intersector COMPUTES (rounding included) must stay inside the box */
        double pad = 1e-5 + 1e-9 * std::max(std::fabs(lo[k]), std::fabs(hi[k]));
        lo[k] -= pad;
        hi[k] += pad;
    }
}

struct BvhBuilder
{
    std::vector<BuildPrim> prims;
    std::vector<BvhNode>   nodes;
    std::vector<uint32_t>  order;
    int LEAF = 1; /* surfaces per leaf: ONE, which is what the kernels' leaf steps are written for (the reference packs a count <= 8 in 3 bits).
                     Config 5, trace stage: 757 ms with 1, 855 with 2, 948 with 4 */
    int max_depth = 0;    /* deepest level holding a node: the traversal pushes at most one entry per level */
    double pad32 = 0.0;   /* extra padding of the STORED boxes that pays for testing them in f32 (drt_kernels.h, Ray32) */
    double extent = 0.0;  /* largest |coordinate| of the surfaces' boxes and of the camera */

    void bounds(size_t b, size_t e, double lo[3], double hi[3]) const
    {
        for (int k = 0; k < 3; k += 1) { lo[k] = HUGE_VAL; hi[k] = -HUGE_VAL; }
        for (size_t i = b; i < e; i += 1)
            for (int k = 0; k < 3; k += 1)
            {
                lo[k] = std::min(lo[k], prims[i].lo[k]);
                hi[k] = std::max(hi[k], prims[i].hi[k]);
            }
    }
    /* fills child slot c of node `parent` with the subtree over prims [b, e) */
    void set_child(int parent, int c, size_t b, size_t e, int depth)
    {
        double lo[3], hi[3];
        bounds(b, e, lo, hi);
        max_depth = std::max(max_depth, depth + 1);
        for (int k = 0; k < 3; k += 1)
        {
            lo[k] -= pad32;
            hi[k] += pad32;
            /* outward to f32: the stored box must contain the (already padded) f64 box */
            float fl = (float)lo[k], fh = (float)hi[k];
            if ((double)fl > lo[k]) fl = std::nextafterf(fl, -INFINITY);
            if ((double)fh < hi[k]) fh = std::nextafterf(fh, INFINITY);
            nodes[parent].lo[c][k] = fl;
            nodes[parent].hi[c][k] = fh;
        }
        if (e - b <= (size_t)LEAF)
        {
            nodes[parent].child[c] = -2 - ((int32_t)order.size() * 8 + ((int32_t)(e - b) - 1)); /* bvh_leaf_ref(first slot, count) */
            nodes[parent].count[c] = (int32_t)(e - b);
            for (size_t i = b; i < e; i += 1) order.push_back(prims[i].idx);
            return;
        }
        int me = (int)nodes.size();
        nodes.push_back(BvhNode());
        nodes[parent].child[c] = me;
        nodes[parent].count[c] = 0;
        split(me, b, e, depth + 1);
    }
    static double half_area(const double lo[3], const double hi[3])
    {
        double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    }
    /* Binned surface-area heuristic (32 bins per axis, all three axes): the split that minimises
     * area(left)*n(left) + area(right)*n(right); falls back to the median along the widest axis when the
     * centroids do not separate. Only the amount of pruning depends on this, never a result. */
    void split(int node, size_t b, size_t e, int depth)
    {
        const int BINS = 32;
        double clo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, chi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        for (size_t i = b; i < e; i += 1)
            for (int k = 0; k < 3; k += 1)
            {
                clo[k] = std::min(clo[k], prims[i].c[k]);
                chi[k] = std::max(chi[k], prims[i].c[k]);
            }
        int best_axis = -1, best_bin = -1;
        double best_cost = HUGE_VAL;
        /* SAH trees have no depth bound of their own, and the traversal stacks hold BVH_STACK entries, one per level at most.
         * A median-split subtree over m surfaces is at most 1 + ceil(log2 m) levels deep, so the SAH may split this node only
         * while a median-split subtree below its children would still fit. */
        int log2m = 0;
        while (((size_t)1 << log2m) < e - b) log2m += 1;
        if (!getenv("DRT_BVH_MEDIAN") && depth + 2 + log2m < BVH_STACK)
            for (int axis = 0; axis < 3; axis += 1)
            {
                double ext = chi[axis] - clo[axis];
                if (!(ext > 0.0)) continue;
                double blo[BINS][3], bhi[BINS][3];
                size_t cnt[BINS];
                for (int k = 0; k < BINS; k += 1)
                {
                    cnt[k] = 0;
                    for (int a = 0; a < 3; a += 1) { blo[k][a] = HUGE_VAL; bhi[k][a] = -HUGE_VAL; }
                }
                for (size_t i = b; i < e; i += 1)
                {
                    int k = std::min(BINS - 1, (int)((prims[i].c[axis] - clo[axis]) / ext * BINS));
                    cnt[k] += 1;
                    for (int a = 0; a < 3; a += 1)
                    {
                        blo[k][a] = std::min(blo[k][a], prims[i].lo[a]);
                        bhi[k][a] = std::max(bhi[k][a], prims[i].hi[a]);
                    }
                }
                /* sweep: right-side areas from the back, then left side from the front */
                double r_area[BINS];
                size_t r_cnt[BINS];
                double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
                size_t n = 0;
                for (int k = BINS - 1; k > 0; k -= 1)
                {
                    if (cnt[k]) for (int a = 0; a < 3; a += 1) { lo[a] = std::min(lo[a], blo[k][a]); hi[a] = std::max(hi[a], bhi[k][a]); }
                    n += cnt[k];
                    r_area[k] = n ? half_area(lo, hi) : 0.0;
                    r_cnt[k] = n;
                }
                for (int a = 0; a < 3; a += 1) { lo[a] = HUGE_VAL; hi[a] = -HUGE_VAL; }
                n = 0;
                for (int k = 0; k + 1 < BINS; k += 1) /* split after bin k */
                {
                    if (cnt[k]) for (int a = 0; a < 3; a += 1) { lo[a] = std::min(lo[a], blo[k][a]); hi[a] = std::max(hi[a], bhi[k][a]); }
                    n += cnt[k];
                    if (n == 0 || r_cnt[k + 1] == 0) continue;
                    double cost = half_area(lo, hi) * (double)n + r_area[k + 1] * (double)r_cnt[k + 1];
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = k; }
                }
            }
        size_t mid;
        if (best_axis >= 0)
        {
            const int axis = best_axis, bin = best_bin;
            const double lo0 = clo[axis], ext = chi[axis] - clo[axis];
            auto it = std::stable_partition(prims.begin() + b, prims.begin() + e, [=](const BuildPrim &x) {
                return std::min(BINS - 1, (int)((x.c[axis] - lo0) / ext * BINS)) <= bin;
            });
            mid = (size_t)(it - prims.begin());
        }
        else
        {
            int axis = 0;
            for (int k = 1; k < 3; k += 1) if (chi[k] - clo[k] > chi[axis] - clo[axis]) axis = k;
            mid = (b + e) / 2;
            std::nth_element(prims.begin() + b, prims.begin() + mid, prims.begin() + e,
                             [axis](const BuildPrim &x, const BuildPrim &y) { return x.c[axis] < y.c[axis] || (x.c[axis] == y.c[axis] && x.idx < y.idx); });
        }
        set_child(node, 0, b, mid, depth);
        set_child(node, 1, mid, e, depth);
    }
    /* `reach`: the largest |coordinate| a ray origin outside the surfaces can have (the camera) */
    void build(const drt_scene *scene, double reach)
    {
        extent = reach;
        for (uint32_t i = 0; i < scene->num_surfaces; i += 1)
        {
            const drt_surface &s = scene->surfaces[i];
            if (s.type != DRT_GEO_SPHERE && s.type != DRT_GEO_PLANE) continue; /* points are never intersected */
            BuildPrim p;
            prim_bounds(s, p.lo, p.hi);
            for (int k = 0; k < 3; k += 1)
            {
                p.c[k] = 0.5 * (p.lo[k] + p.hi[k]);
                if (std::fabs(p.lo[k]) < 1e299) extent = std::max(extent, std::fabs(p.lo[k]));
                if (std::fabs(p.hi[k]) < 1e299) extent = std::max(extent, std::fabs(p.hi[k]));
            }
            p.idx = i;
            prims.push_back(p);
        }
        /* the f32 box test moves a slab plane by < 6 * 2^-24 * extent (drt_kernels.h, Ray32): pad by 2^-19 * extent, 5x that */
        pad32 = std::ldexp(extent, -19);
        nodes.push_back(BvhNode());
        nodes[0].count[0] = nodes[0].count[1] = -1;
        nodes[0].child[0] = nodes[0].child[1] = BVH_DONE; /* no child */
        if (prims.empty()) return;
        if (prims.size() <= (size_t)LEAF) set_child(0, 0, 0, prims.size(), 0);
        else split(0, 0, prims.size(), 0);
    }
};

static void shade_sets(uint32_t S, uint32_t *n_sets, uint32_t *tail_first, uint32_t *tail_count);

/* what eval_coefficients must compute for a list holding BDSF b (DevMaterial.needs) */
static uint32_t bdsf_needs(uint32_t b)
{
    if (b == DRT_BDSF_bp_glossy_bdsf) return NEED_GLOSSY;
    if (b == DRT_BDSF_mirror_bdsf || b == DRT_BDSF_fs_conductor_bdsf || b == DRT_BDSF_fs_dielectric_reflectance_bdsf) return NEED_EQR;
    if (b == DRT_BDSF_fs_dielectric_transmittance_bdsf) return NEED_EQT;
    if (b == DRT_BDSF_ct_conductor_bdsf) return NEED_CT;
    return 0u;
}

/* Can the closed shade instantiation (csrc/drt_kernels.h, shade_pixels<CLOSED>) replay this scene? Every material -- used by a surface
 * or not -- must list nothing or exactly one of the five lists that have straight-line code: the two-lobe plastic, {mirror},
 * {dielectric reflectance, dielectric transmittance}, {smooth conductor}, {rough conductor}. A permutation, a sublist or a superset of
 * one of them is another list: the general instantiation's. And a material that lists NOTHING must never be shaded: the trace kernel
 * records a vertex for every hit on a surface whose material is no black body, the general list sums such a vertex to zero, and the
 * closed code has no form for the empty list (it would take it for the rough conductor or the plastic). So no surface's material may
 * be one that is no black body and lists nothing (smat: the material of every surface). Surfaces keep their materials and
 * materials their lists and their is_black_body for a context's life (update_surfaces, materials_check), so this is decided once. */
static bool closed_lists(const DevMaterial *mats, uint32_t n, const uint32_t *smat, uint32_t n_surf)
{
    for (uint32_t i = 0; i < n_surf; i += 1)
        if (!mats[smat[i]].is_black_body && mats[smat[i]].num_bdsfs == 0u) return false;
    for (uint32_t i = 0; i < n; i += 1)
    {
        const DevMaterial &m = mats[i];
        const bool one = m.num_bdsfs == 1u && (m.bdsf_packed == DRT_LIST_MIRROR || m.bdsf_packed == DRT_LIST_CONDUCTOR || m.bdsf_packed == DRT_LIST_GGX);
        const bool two = m.num_bdsfs == 2u && (m.bdsf_packed == DRT_LIST_PLASTIC || m.bdsf_packed == DRT_LIST_GLASS);
        if (m.num_bdsfs != 0u && !one && !two) return false;
    }
    return true;
}

static int build_device_scene(drt_context *ctx, const drt_scene *scene, double reach)
{
    const uint32_t S = scene->num_wavelengths;
    const uint32_t n_surf = scene->num_surfaces;
    if (S == 0 || scene->num_spds == 0 || !scene->spds) return fail(-2, "scene has no spectral tables");
    if (scene->base_material >= scene->num_materials || scene->escape_material >= scene->num_materials)
        return fail(-2, "base/escape material index out of range");

    DevScene &d = ctx->dsc;
    d.n_surf = n_surf;
    d.n_mat = scene->num_materials;
    d.S = S;
    d.n_spd = scene->num_spds;
    d.base_mat = scene->base_material;
    d.escape_mat = scene->escape_material;
    /* value_at_wl(., trans_wl = 630), src/spectrum.c:150-162 and src/daily_ray_trace.c:381 */
    d.trans_wl = 630.0;
    d.trans_i0 = (uint32_t)((d.trans_wl - scene->min_wavelength) / scene->wavelength_interval);
    if (d.trans_i0 + 1 >= S) return fail(-2, "wavelength grid does not bracket trans_wl = 630 nm");
    d.trans_w0 = scene->min_wavelength + d.trans_i0 * scene->wavelength_interval;
    d.trans_w1 = scene->min_wavelength + (d.trans_i0 + 1) * scene->wavelength_interval;

    std::vector<double> surf((size_t)SF_COUNT * n_surf, 0.0);
    std::vector<uint32_t> stype(n_surf), smat(n_surf);
    std::vector<double> lights;
    std::vector<uint32_t> ltype, lmat;
    std::vector<uint32_t> light_surfaces;
    for (uint32_t i = 0; i < n_surf; i += 1)
    {
        const drt_surface &s = scene->surfaces[i];
        if (s.material >= scene->num_materials) return fail(-2, "surface %u: material index out of range", i);
        stype[i] = s.type;
        smat[i] = s.material;
        surf[(size_t)SF_PX * n_surf + i] = s.position[0];
        surf[(size_t)SF_PY * n_surf + i] = s.position[1];
        surf[(size_t)SF_PZ * n_surf + i] = s.position[2];
        surf[(size_t)SF_RADIUS * n_surf + i] = s.radius;
        if (s.type == DRT_GEO_PLANE)
        {
            /* |u|, |v|, u/|u|, v/|v|: what line_plane_intersection recomputes per ray (src/geometry.c:166-170) */
            double ul = h_length(s.u), vl = h_length(s.v);
            surf[(size_t)SF_NX * n_surf + i] = s.normal[0];
            surf[(size_t)SF_NY * n_surf + i] = s.normal[1];
            surf[(size_t)SF_NZ * n_surf + i] = s.normal[2];
            for (int k = 0; k < 3; k += 1)
            {
                surf[(size_t)(SF_UNX + k) * n_surf + i] = s.u[k] / ul;
                surf[(size_t)(SF_VNX + k) * n_surf + i] = s.v[k] / vl;
            }
            surf[(size_t)SF_ULEN * n_surf + i] = ul;
            surf[(size_t)SF_VLEN * n_surf + i] = vl;
        }
        if (scene->materials[s.material].is_emissive) light_surfaces.push_back(i);
    }
    const uint32_t n_lights = (uint32_t)light_surfaces.size();
    d.n_lights = n_lights;
    lights.assign((size_t)LF_COUNT * std::max<uint32_t>(n_lights, 1), 0.0);
    ltype.resize(n_lights);
    lmat.resize(n_lights);
    for (uint32_t l = 0; l < n_lights; l += 1)
    {
        const drt_surface &s = scene->surfaces[light_surfaces[l]];
        ltype[l] = s.type;
        lmat[l] = s.material;
        for (int k = 0; k < 3; k += 1)
        {
            lights[(size_t)(LF_PX + k) * n_lights + l] = s.position[k];
            lights[(size_t)(LF_UX + k) * n_lights + l] = s.u[k];
            lights[(size_t)(LF_VX + k) * n_lights + l] = s.v[k];
        }
        lights[(size_t)LF_RADIUS * n_lights + l] = s.radius;
        double pdf = 1.0; /* src/daily_ray_trace.c:292, :304, :314 */
        if (s.type == DRT_GEO_SPHERE) pdf = ((4.0 * DRT_PI) * s.radius) * s.radius;
        else if (s.type == DRT_GEO_PLANE)
        {
            double c[3] = {s.u[1] * s.v[2] - s.u[2] * s.v[1], s.u[2] * s.v[0] - s.u[0] * s.v[2], s.u[0] * s.v[1] - s.u[1] * s.v[0]};
            pdf = h_length(c);
        }
        lights[(size_t)LF_PDF * n_lights + l] = pdf;
    }

    std::vector<double> spds(scene->spds, scene->spds + (size_t)scene->num_spds * S);
    std::vector<SpdRowDesc> &desc = ctx->spd_desc; /* how every row is made: what drt_update_spectra derives the table from again */
    desc.clear();
    for (uint32_t r = 0; r < scene->num_spds; r += 1) desc.push_back(SpdRowDesc{SPD_ROW_SCENE, (int32_t)r, -1, -1});
    std::map<int32_t, uint32_t> diffuse_pi_row;
    /* the zero row is appended last; derived rows go between: reserve its index now */
    uint32_t n_diffuse = 0;
    {
        std::map<int32_t, int> seen;
        for (uint32_t i = 0; i < scene->num_materials; i += 1)
            if (scene->materials[i].diffuse_spd >= 0 && !seen[scene->materials[i].diffuse_spd]++) n_diffuse += 1;
    }
    /* Rows tabulated per pair of media for the Fresnel terms (drt_device.h, *_reflectance_sel; drt_kernels.h, PAIR_*): a material
     * whose list holds dielectric Fresnel functions gets one row (rel_sq) for rays entering it from the base material and one for
     * rays leaving it; one that holds conductor functions two rows (cA, cB) for rays arriving from the base material. A list
     * with both kinds gets none (the shade kernel tells the kind from the pair field, not per function). */
    auto fresnel_kind = [&](const drt_material &m) -> int { /* 0 none or mixed, 1 dielectric, 2 conductor */
        bool d = false, c = false;
        for (uint32_t j = 0; j < std::min<uint32_t>(m.num_bdsfs, DRT_MAX_BDSFS); j += 1)
        {
            const uint32_t b = m.bdsfs[j];
            d = d || b == DRT_BDSF_fs_dielectric_reflectance_bdsf || b == DRT_BDSF_fs_dielectric_transmittance_bdsf;
            c = c || b == DRT_BDSF_fs_conductor_bdsf || b == DRT_BDSF_ct_conductor_bdsf;
        }
        if (getenv("DRT_NO_PAIR_ROWS")) return 0; /* A/B knob of the parity tests: every term from ir, tr, te */
        return (d && !c) ? 1 : (c && !d) ? 2 : 0;
    };
    uint32_t n_pair_rows = 0;
    for (uint32_t i = 0; i < scene->num_materials; i += 1) n_pair_rows += 2u * (uint32_t)(fresnel_kind(scene->materials[i]) != 0);
    const uint32_t zero_row = scene->num_spds + n_diffuse + n_pair_rows;
    if (zero_row >= PAIR_CONDUCTOR) n_pair_rows = 0; /* row numbers must fit below the kind bit: (never with real scenes) no pair rows then */
    std::vector<DevMaterial> mats(scene->num_materials);
    for (uint32_t i = 0; i < scene->num_materials; i += 1)
    {
        const drt_material &m = scene->materials[i];
        DevMaterial &dm = mats[i];
        memset(&dm, 0, sizeof(dm));
        dm.is_black_body = m.is_black_body;
        dm.is_emissive = m.is_emissive;
        dm.num_bdsfs = std::min<uint32_t>(m.num_bdsfs, DRT_MAX_BDSFS);
        dm.dir_func = m.dir_func;
        const int32_t idx[6] = {m.emission_spd, m.diffuse_spd, m.glossy_spd, m.mirror_spd, m.refract_spd, m.extinct_spd};
        for (int k = 0; k < 6; k += 1)
            if (idx[k] >= (int32_t)scene->num_spds) return fail(-2, "material %u: SPD index out of range", i);
        /* device rows: scene rows as they are; a missing spectrum -> the all-zero row; diffuse -> its derived
         * diffuse * (1/PI) row (bp_diffuse_bdsf's first product, src/bdsf.c:107, is a per-material constant) */
        auto row = [&](int32_t i) { return i >= 0 ? i : (int32_t)zero_row; };
        dm.emission_spd = row(m.emission_spd); dm.glossy_spd = row(m.glossy_spd);
        dm.mirror_spd = row(m.mirror_spd); dm.refract_spd = row(m.refract_spd); dm.extinct_spd = row(m.extinct_spd);
        dm.diffuse_spd = (int32_t)zero_row;
        if (m.diffuse_spd >= 0)
        {
            auto it = diffuse_pi_row.find(m.diffuse_spd);
            if (it == diffuse_pi_row.end())
            {
                const double inv_pi = 1.0 / DRT_PI;
                uint32_t r = (uint32_t)(spds.size() / S);
                for (uint32_t k = 0; k < S; k += 1) spds.push_back(scene->spds[(size_t)m.diffuse_spd * S + k] * inv_pi);
                desc.push_back(SpdRowDesc{SPD_ROW_DIFFUSE_PI, m.diffuse_spd, -1, -1});
                it = diffuse_pi_row.emplace(m.diffuse_spd, r).first;
            }
            dm.diffuse_spd = (int32_t)it->second;
        }
        dm.shininess = m.shininess;
        dm.roughness = m.roughness;
        if (m.refract_spd >= 0)
        {
            dm.refract_i0 = scene->spds[(size_t)m.refract_spd * S + d.trans_i0];
            dm.refract_i1 = scene->spds[(size_t)m.refract_spd * S + d.trans_i0 + 1];
        }
        for (uint32_t j = 0; j < dm.num_bdsfs; j += 1)
        {
            uint32_t b = m.bdsfs[j];
            if (b >= DRT_NUM_BDSFS) return fail(-2, "material %u: unknown bdsf id %u", i, b);
            dm.bdsfs[j] = b;
            dm.bdsf_packed |= (uint64_t)b << (4 * j);
            dm.needs |= bdsf_needs(b);
        }
        if (dm.num_bdsfs == 2 && dm.bdsfs[0] == DRT_BDSF_bp_diffuse_bdsf && dm.bdsfs[1] == DRT_BDSF_bp_glossy_bdsf) dm.vertex_flags = FLAG_PLASTIC;
        dm.pair_out = dm.pair_in = PAIR_NONE;
        const int kind = n_pair_rows ? fresnel_kind(m) : 0;
        if (kind)
        {
            /* a spectrum that is not given reads as zeros, as everywhere (the table's all-zero row) */
            const drt_material &bm = scene->materials[scene->base_material];
            auto at = [&](int32_t spd, uint32_t k) { return spd >= 0 ? scene->spds[(size_t)spd * S + k] : 0.0; };
            const uint32_t r0 = (uint32_t)(spds.size() / S);
            if (kind == 1)
            {
                /* rel_sq = (ir / tr) (ir / tr), src/bdsf.c:52-56: entering (ir the base material's, tr this one's), then leaving */
                for (uint32_t k = 0; k < S; k += 1) { const double rel = at(bm.refract_spd, k) / at(m.refract_spd, k); spds.push_back(rel * rel); }
                for (uint32_t k = 0; k < S; k += 1) { const double rel = at(m.refract_spd, k) / at(bm.refract_spd, k); spds.push_back(rel * rel); }
                desc.push_back(SpdRowDesc{SPD_ROW_REL_SQ, bm.refract_spd, m.refract_spd, -1});
                desc.push_back(SpdRowDesc{SPD_ROW_REL_SQ, m.refract_spd, bm.refract_spd, -1});
                dm.pair_out = (uint16_t)r0;
                dm.pair_in = (uint16_t)(r0 + 1u);
            }
            else
            {
                /* cA = rr_sq - re_sq, cB = 4 rr_sq re_sq with rr = tr / ir, re = te / ir, src/bdsf.c:84-91 */
                std::vector<double> cB(S);
                for (uint32_t k = 0; k < S; k += 1)
                {
                    const double ir = at(bm.refract_spd, k), rr = at(m.refract_spd, k) / ir, re = at(m.extinct_spd, k) / ir;
                    const double rr_sq = rr * rr, re_sq = re * re;
                    spds.push_back(rr_sq - re_sq);
                    cB[k] = 4.0 * rr_sq * re_sq;
                }
                spds.insert(spds.end(), cB.begin(), cB.end());
                desc.push_back(SpdRowDesc{SPD_ROW_CONDUCTOR_A, m.refract_spd, m.extinct_spd, bm.refract_spd});
                desc.push_back(SpdRowDesc{SPD_ROW_CONDUCTOR_B, m.refract_spd, m.extinct_spd, bm.refract_spd});
                dm.pair_out = (uint16_t)(r0 | PAIR_CONDUCTOR);
            }
        }
        if (!m.is_black_body && dm.dir_func >= DRT_NUM_DIRFS) return fail(-2, "material %u: unknown dir_func id %u", i, dm.dir_func);
    }
    spds.resize((size_t)(zero_row + 1) * S, 0.0); /* + the all-zero row */
    desc.resize((size_t)zero_row + 1, SpdRowDesc{SPD_ROW_ZERO, -1, -1, -1});
    d.n_spd = zero_row + 1;

    int rc;
    if ((rc = upload(ctx, surf, &d.surf))) return rc;
    if ((rc = upload(ctx, stype, &d.surf_type))) return rc;
    if ((rc = upload(ctx, smat, &d.surf_mat))) return rc;
    if ((rc = upload(ctx, lights, &d.lights))) return rc;
    if ((rc = upload(ctx, ltype, &d.light_type))) return rc;
    if ((rc = upload(ctx, lmat, &d.light_mat))) return rc;
    ctx->light0_em_spd = n_lights ? ((uint32_t)mats[lmat[0]].emission_spd & 0xFFFFu) : 0u; /* what the trace kernel writes into light 0's blocks */
    if ((rc = upload(ctx, mats, &d.mats))) return rc;
    ctx->host_mats = mats;
    if ((rc = upload(ctx, spds, &d.spds))) return rc;

    ctx->cmf_rw = scene->cmf_rw; ctx->cmf_x = scene->cmf_x; ctx->cmf_y = scene->cmf_y; ctx->cmf_z = scene->cmf_z;
    ctx->interval = scene->wavelength_interval;
    if (std::max(std::max(ctx->cmf_rw, ctx->cmf_x), std::max(ctx->cmf_y, ctx->cmf_z)) >= scene->num_spds)
        return fail(-2, "colour-matching SPD index out of range");

    /* LDS budgets: keep the scene in LDS when it leaves room for >= 2 workgroups per CU */
    ctx->trace_lds = trace_lds_bytes(n_surf, n_lights, scene->num_materials);
    /* small scenes: whole scan out of LDS; large scenes: tables stay in HBM/L2 and a BVH prunes the scan */
    ctx->scene_in_lds = ctx->trace_lds <= 64 * 1024 && n_surf <= 96 && !getenv("DRT_FORCE_BVH");
    ctx->use_bvh = !ctx->scene_in_lds; /* (round 1's brute-force scan from HBM, DRT_NO_BVH, is gone: the two BVH kernels are the only path for such scenes) */
    d.bvh_nodes = nullptr;
    d.bvh_leaf = nullptr;
    if (ctx->use_bvh)
    {
        BvhBuilder bb;
        bb.build(scene, reach);
        /* the traversal stacks hold BVH_STACK entries, one per level at most, and push unchecked */
        if (bb.max_depth > BVH_STACK) return fail(-2, "BVH of %zu surfaces is %d levels deep, the traversal stack holds %d", bb.prims.size(), bb.max_depth, BVH_STACK);
        /* the f32 box test multiplies coordinates by 1/d capped at 2^100 (drt_kernels.h, bvh_inv32) */
        if (!(bb.extent < 134217728.0)) return fail(-2, "scene or camera coordinates reach %g: the hierarchy's f32 box test holds up to 2^27", bb.extent);
        std::vector<BvhLeafPrim> leaf(std::max<size_t>(bb.order.size(), 1));
        memset(leaf.data(), 0, leaf.size() * sizeof(BvhLeafPrim));
        for (size_t k = 0; k < bb.order.size(); k += 1)
        {
            const uint32_t i = bb.order[k];
            leaf[k].index = i;
            leaf[k].type = stype[i];
            for (int f = 0; f < 4; f += 1) leaf[k].f[f] = surf[(size_t)f * n_surf + i]; /* SF_PX, SF_PY, SF_PZ, SF_RADIUS */
            leaf[k].reach32 = INFINITY; /* planes: never "certainly missed" */
            if (stype[i] == DRT_GEO_SPHERE)
            {
                for (int f = 0; f < 3; f += 1) leaf[k].c32[f] = (float)leaf[k].f[f];
                leaf[k].reach32 = bvh_sphere_reach32(leaf[k].f[3], bb.extent);
            }
        }
        if ((rc = upload(ctx, bb.nodes, &d.bvh_nodes))) return rc;
        if ((rc = upload(ctx, leaf, &d.bvh_leaf))) return rc;
        ctx->h_nodes = bb.nodes;
        ctx->h_order = bb.order;
        ctx->hb_depth = (uint32_t)bb.max_depth;
        ctx->extent = bb.extent;
    }
    if (!ctx->scene_in_lds) ctx->trace_lds = 0;
    ctx->spds_in_lds = (size_t)d.n_spd * S * 8 <= 64 * 1024;
    /* The tail wavelengths in the trace kernel (csrc/drt_kernels.h, drt_trace_kernel<true, true>): scenes scanned out of LDS with one
     * light and a tail of at most 8 wavelengths, when the table's tail columns and the waves' running values ([2 R + 1][64 lanes] each)
     * fit beside the scene. Paths of two-lobe plastic and mirror vertices (and those without a vertex) are carried there; where
     * every surface is a light, a black body, plastic or a mirror that is EVERY path, and the shade kernel's tail pass has nothing
     * to replay (tail_all_staged). With glass or gold in the scene the paths that touch them stay with the tail pass, as tasks.
     * The rule's 48 KB is of the scene, the table's tail columns and the running values; the lanes' rows (TRACE_LW_*) and the vignette
     * row, 6 KB, are not counted in it, so that a scene takes the kernel it took before they existed. Up to 47 KB of the rule's
     * quantity three workgroups still share a CU's 160 KB. */
    {
        uint32_t sets = 0, tf = 0, tc = 0;
        shade_sets(S, &sets, &tf, &tc);
        const size_t extra = (size_t)d.n_spd * tc * 8 + (size_t)(TRACE_BLOCK / 64) * (2 * tc + 1) * 64 * 8; /* + 1: the vignette row */
        /* every list of every material (used by a surface or not: a ray can only meet a surface's, but the check is cheap) */
        ctx->simple_bdsfs = !getenv("DRT_NO_SIMPLE_SHADE");
        ctx->no_fixed_lists = getenv("DRT_NO_FIXED_LISTS") != nullptr; /* A/B: the main pass's mirror / glass / smooth-conductor vertices through the general list */
        for (uint32_t i = 0; i < scene->num_materials; i += 1)
            for (uint32_t j = 0; j < mats[i].num_bdsfs; j += 1)
            {
                const uint32_t b = mats[i].bdsfs[j];
                if (b != DRT_BDSF_bp_diffuse_bdsf && b != DRT_BDSF_bp_glossy_bdsf && b != DRT_BDSF_mirror_bdsf) ctx->simple_bdsfs = false;
            }
        ctx->no_closed_shade = getenv("DRT_NO_CLOSED_SHADE") != nullptr; /* A/B: the general instantiation where the closed one would run */
        ctx->closed_lists = closed_lists(mats.data(), scene->num_materials, smat.data(), n_surf);
        bool all_simple = true;
        for (uint32_t i = 0; i < n_surf; i += 1)
        {
            const DevMaterial &m = mats[smat[i]];
            const bool mirror_only = m.num_bdsfs == 1u && m.bdsfs[0] == DRT_BDSF_mirror_bdsf;
            if (!(m.is_black_body || (m.vertex_flags & FLAG_PLASTIC) || mirror_only)) all_simple = false;
        }
        /* DRT_TRACE_TAIL: 0 = never (every path's tail through the shade kernel's tail pass), 2 = only in scenes where every path can be
         * carried (round 2's rule); default: whenever the kernel can run -- paths that meet glass or gold stay with the tail pass, which
         * takes them as tasks while the others, three quarters and more, cost it nothing */
        const char *e = getenv("DRT_TRACE_TAIL");
        /* the rule's 48 KB stays what it was of: the lanes' rows and the vignette row (6 KB) come on top */
        const size_t lane_rows = (size_t)(TRACE_BLOCK / 64) * (TRACE_LANE_ROWS + 1) * 64 * 8;
        ctx->trace_tail = ctx->scene_in_lds && sets == 1 && tc > 0 && tc <= 8 && n_lights == 1 && ctx->trace_lds + extra - lane_rows <= 48 * 1024 && !(e && *e == '0') &&
                          (all_simple || !(e && *e == '2'));
        ctx->tail_all_staged = ctx->trace_tail && all_simple;
        /* DRT_TAIL_RESUME=0: paths the trace kernel stops carrying are replayed from vertex 0 (the parity tests' A/B); it travels as a null
         * tail_resume pointer in both kernels' parameters */
        const char *er = getenv("DRT_TAIL_RESUME");
        ctx->tail_resume = ctx->trace_tail && !ctx->tail_all_staged && !(er && *er == '0');
        if (ctx->trace_tail)
        {
            std::vector<double> cols((size_t)d.n_spd * tc);
            for (uint32_t r = 0; r < d.n_spd; r += 1)
                for (uint32_t j = 0; j < tc; j += 1) cols[(size_t)r * tc + j] = spds[(size_t)r * S + tf + j];
            if ((rc = upload(ctx, cols, &ctx->d_spd_tail))) return rc;
            ctx->trace_lds += extra;
        }
    }
    return 0;
}

static bool shade_simple(const drt_context *ctx) { return ctx->simple_bdsfs && ctx->spds_in_lds && ctx->shade_sets == 1; }

/* DARK or not, per launch: a windowed pair (the live window is open and the launch has no pixel list) goes by the window's vertices
 * per path, every other launch by the whole tile's -- so a whole-tile or list launch of a context that has a window runs what it ran
 * before there was one. Same film either way. */
static bool shade_dark(const drt_context *ctx, const ShadeParams &sp)
{
    return (ctx->win_open && !sp.pixel_list) ? ctx->dark_skip_win : ctx->dark_skip;
}

/* The closed instantiation is taken for a context's dense launches (an adaptive round's pixel list keeps the general one) when
 *   - every material's list is covered and no surface's material is a non-black body that lists nothing (closed_lists()), and the
 *     scene is not SIMPLE's (which is leaner still),
 *   - neither DRT_NO_CLOSED_SHADE nor DRT_NO_FIXED_LISTS was set when the context was created,
 *   - the S wavelengths are one set per lane (with or without a packed tail) and the SPD table is in LDS,
 *   - the film is spectral (the XYZ film keeps the general instantiation).
 * Nothing else is asked: lights beyond the first, vertices beyond the prefetched records and records wider than a register go through
 * plastic_vertex's and fixed_vertex's own block-by-block paths, which the closed code keeps. */
static bool shade_closed(const drt_context *ctx)
{
    return ctx->closed_lists && !ctx->no_closed_shade && !ctx->no_fixed_lists && !shade_simple(ctx) && ctx->spds_in_lds && ctx->shade_sets == 1 && !ctx->xyz_mode;
}

/* ... and of the closed kernel's two forms the one with headers and one record slot in LDS, five waves per SIMD (create_impl decides) */
static bool shade_closed_lds(const drt_context *ctx) { return DRT_SHADE_CLOSED_LDS_HEADERS != 0 && ctx->closed_lds && shade_closed(ctx); }
/* ... and of that form the one in workgroups of 512 lanes with one table for eight waves, six waves per SIMD (create_impl decides) */
static bool shade_closed_lds6(const drt_context *ctx) { return ctx->closed_lds6 && shade_closed_lds(ctx); }
/* a shade launch's workgroup, in waves, and the cap of its persistent grid (`list`: an adaptive round, the general LIST instantiation) */
static uint32_t shade_launch_waves(const drt_context *ctx, bool list) { return !list && shade_closed_lds6(ctx) ? SHADE_WAVES_CLOSED_LDS6 : SHADE_WAVES; }
static uint32_t shade_launch_grid_cap(const drt_context *ctx, bool list) { return (uint32_t)(!list && shade_closed_lds6(ctx) ? ctx->shade_grid_cap6 : ctx->shade_grid_cap); }

template <int NSETS, bool XYZ, bool LIST>
static int launch_shade_mode(drt_context *ctx, uint32_t grid, const ShadeParams &sp, double *const film[3])
{
    if (NSETS == 1 && !XYZ && !LIST && shade_closed(ctx))
    {
#define DRT_LAUNCH_CLOSED(KERNEL, DARK, LDS_BYTES)                                                                                                 \
    hipLaunchKernelGGL((KERNEL<DARK>), dim3(grid), dim3(SHADE_BLOCK), LDS_BYTES, ctx->stream, ctx->dsc, sp, ctx->d_records, \
                       ctx->d_headers, film[0], film[1], film[2], ctx->d_counters + DRT_NUM_COUNTERS + 1)
#if DRT_SHADE_CLOSED_LDS_HEADERS
        if (shade_closed_lds6(ctx))
        {
#define DRT_LAUNCH_CLOSED6(DARK)                                                                                                                   \
    hipLaunchKernelGGL((drt_shade_kernel_closed_lds6<DARK>), dim3(grid), dim3(SHADE_BLOCK_CLOSED_LDS6), ctx->shade_lds_closed6, ctx->stream, ctx->dsc, sp, \
                       ctx->d_records, ctx->d_headers, film[0], film[1], film[2], ctx->d_counters + DRT_NUM_COUNTERS + 1)
            if (shade_dark(ctx, sp)) DRT_LAUNCH_CLOSED6(true);
            else DRT_LAUNCH_CLOSED6(false);
#undef DRT_LAUNCH_CLOSED6
            return 0;
        }
        if (shade_closed_lds(ctx))
        {
            if (shade_dark(ctx, sp)) DRT_LAUNCH_CLOSED(drt_shade_kernel_closed_lds, true, ctx->shade_lds_closed);
            else DRT_LAUNCH_CLOSED(drt_shade_kernel_closed_lds, false, ctx->shade_lds_closed);
            return 0;
        }
#endif
        if (shade_dark(ctx, sp)) DRT_LAUNCH_CLOSED(drt_shade_kernel_closed, true, ctx->shade_lds);
        else DRT_LAUNCH_CLOSED(drt_shade_kernel_closed, false, ctx->shade_lds);
#undef DRT_LAUNCH_CLOSED
        return 0;
    }
#define DRT_LAUNCH_SHADE(LDS, DARK, SIMPLE)                                                                                                       \
    hipLaunchKernelGGL((drt_shade_kernel<NSETS, LDS, XYZ, DARK, SIMPLE, LIST>), dim3(grid), dim3(SHADE_BLOCK), ctx->shade_lds, ctx->stream, ctx->dsc, sp, \
                       ctx->d_records, ctx->d_headers, film[0], film[1], film[2], ctx->d_counters + DRT_NUM_COUNTERS + 1)
    /* SIMPLE: scenes without a Fresnel function, one wavelength set per lane, tables in LDS (shade_simple()) */
    if (NSETS == 1 && shade_simple(ctx))
    {
        if (shade_dark(ctx, sp)) DRT_LAUNCH_SHADE(true, true, (NSETS == 1));
        else DRT_LAUNCH_SHADE(true, false, (NSETS == 1));
    }
    else if (ctx->spds_in_lds && shade_dark(ctx, sp)) DRT_LAUNCH_SHADE(true, true, false);
    else if (ctx->spds_in_lds) DRT_LAUNCH_SHADE(true, false, false);
    else if (shade_dark(ctx, sp)) DRT_LAUNCH_SHADE(false, true, false);
    else DRT_LAUNCH_SHADE(false, false, false);
#undef DRT_LAUNCH_SHADE
    return 0;
}

template <int NSETS>
static int launch_shade_sets(drt_context *ctx, uint32_t grid, const ShadeParams &sp, double *const film[3])
{
    if (sp.pixel_list) return launch_shade_mode<NSETS, false, true>(ctx, grid, sp, film); /* an adaptive round: spectral film only */
    return ctx->xyz_mode ? launch_shade_mode<NSETS, true, false>(ctx, grid, sp, film) : launch_shade_mode<NSETS, false, false>(ctx, grid, sp, film);
}

/* How the S wavelengths map to lanes: n full 64-lane sets, plus (when the remainder is small) a packed tail pass */
static void shade_sets(uint32_t S, uint32_t *n_sets, uint32_t *tail_first, uint32_t *tail_count)
{
    uint32_t full = S / 64, rem = S % 64;
    *tail_first = 0;
    *tail_count = 0;
    if (S <= 64 || rem == 0) *n_sets = (S + 63) / 64;
    else if (rem <= 16 && !getenv("DRT_NO_TAIL_PASS"))
    {
        *n_sets = full;
        *tail_first = 64 * full;
        *tail_count = rem;
    }
    else *n_sets = full + 1;
}

/* film: the three buffers from the first pixel the launch covers on (a launch may cover a range of the tile's rows) */
static int launch_shade(drt_context *ctx, uint32_t grid, const ShadeParams &sp, double *const film[3])
{
    switch (ctx->shade_sets)
    {
        case 1: return launch_shade_sets<1>(ctx, grid, sp, film);
        case 2: return launch_shade_sets<2>(ctx, grid, sp, film);
        case 3: return launch_shade_sets<3>(ctx, grid, sp, film);
        default: return launch_shade_sets<4>(ctx, grid, sp, film);
    }
}

/* The cut pass of one kernel pair (depth cuts bound): drt_depth_cut_kernel over the pair's pixels and samples, behind its shade kernel.
 * pix0: the launch's first pixel in the tile, where its rows of the cut films start. Its queue is word +3 of the pair's work words. */
template <int NCUTS>
static const void *depth_kernel(bool lds) { return lds ? (const void *)drt_depth_cut_kernel<NCUTS, true> : (const void *)drt_depth_cut_kernel<NCUTS, false>; }
static const void *depth_kernel(uint32_t n_cuts, bool lds)
{
    switch (n_cuts)
    {
        case 1: return depth_kernel<1>(lds);
        case 2: return depth_kernel<2>(lds);
        case 3: return depth_kernel<3>(lds);
        case 4: return depth_kernel<4>(lds);
        case 5: return depth_kernel<5>(lds);
        case 6: return depth_kernel<6>(lds);
        case 7: return depth_kernel<7>(lds);
        default: return depth_kernel<8>(lds);
    }
}
static size_t depth_lds_bytes(const drt_context *ctx) { return ctx->spds_in_lds ? (size_t)ctx->dsc.n_spd * ctx->dsc.S * 8 : 0; }

static int launch_depth_cuts(drt_context *ctx, const ShadeParams &sp, uint64_t pix0)
{
    const size_t S = ctx->dsc.S;
    DepthCutParams dp{};
    dp.n_pix = sp.n_pix;
    dp.n_samples = sp.n_samples;
    dp.first_sample = sp.first_sample;
    dp.vertex_words = sp.vertex_words;
    dp.block_words = sp.block_words;
    dp.n_lights = sp.n_lights;
    dp.batch = sp.batch;
    dp.overflow = sp.overflow;
    dp.n_sets = (uint32_t)((S + 63) / 64);
    if (sp.n_pix * dp.n_sets >= 0xFFFFFFFFull) return fail(-1, "tile too large for the depth-cut work queue");
    dp.n_items = (uint32_t)(sp.n_pix * dp.n_sets);
    for (uint32_t c = 0; c < ctx->n_cuts; c += 1)
    {
        dp.depth[c] = ctx->cut_depth[c];
        dp.pixels[c] = ctx->cuts.pixels[c] + pix0 * (S + 1);
        dp.avgs[c] = ctx->cuts.avgs[c] + pix0 * S;
        dp.vars[c] = ctx->cuts.vars[c] + pix0 * S;
    }
    const uint64_t *records = ctx->d_records, *headers = ctx->d_headers;
    unsigned long long *queue = ctx->d_counters + DRT_NUM_COUNTERS + 3;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)dp.n_items + DEPTH_WAVES - 1) / DEPTH_WAVES, (uint64_t)ctx->depth_grid_cap);
    void *args[] = {&ctx->dsc, &dp, &records, &headers, &queue};
    HIP_TRY(hipLaunchKernel(depth_kernel(ctx->n_cuts, ctx->spds_in_lds), dim3(grid), dim3(DEPTH_BLOCK), args, depth_lds_bytes(ctx), ctx->stream));
    return 0;
}

/* The sensor pass of one kernel pair (a sensor bound): drt_sensor_kernel over the pair's pixels and samples, behind its shade kernel.
 * Its queue is the cut pass's word, +3 of the pair's work words: cuts and a sensor are never bound together. */
static const void *sensor_kernel(bool lds) { return lds ? (const void *)drt_sensor_kernel<true> : (const void *)drt_sensor_kernel<false>; }
static size_t sensor_lds_bytes(const drt_context *ctx, uint32_t n, bool lds) { return ((lds ? (size_t)ctx->dsc.n_spd : 0) + n) * ctx->dsc.S * 8; }

/* The bucket pass of one kernel pair (buckets bound): drt_bucket_kernel over the pair's pixels and samples, behind its shade kernel.
 * Its queue is the cut pass's word, +3 of the pair's work words: of cuts, a sensor and buckets only one is ever bound. */
template <int NB>
static const void *bucket_kernel(bool lds) { return lds ? (const void *)drt_bucket_kernel<NB, true> : (const void *)drt_bucket_kernel<NB, false>; }
static const void *bucket_kernel(uint32_t n, bool lds)
{
    switch (n)
    {
        case 1: return bucket_kernel<1>(lds);
        case 2: return bucket_kernel<2>(lds);
        case 3: return bucket_kernel<3>(lds);
        case 4: return bucket_kernel<4>(lds);
        case 5: return bucket_kernel<5>(lds);
        case 6: return bucket_kernel<6>(lds);
        case 7: return bucket_kernel<7>(lds);
        default: return bucket_kernel<8>(lds);
    }
}

static int launch_buckets(drt_context *ctx, const ShadeParams &sp, uint64_t pix0)
{
    const size_t S = ctx->dsc.S;
    BucketParams bp{};
    bp.n_pix = sp.n_pix;
    bp.n_samples = sp.n_samples;
    bp.first_sample = sp.first_sample;
    bp.vertex_words = sp.vertex_words;
    bp.block_words = sp.block_words;
    bp.n_lights = sp.n_lights;
    bp.batch = sp.batch;
    bp.overflow = sp.overflow;
    bp.n_sets = (uint32_t)((S + 63) / 64);
    bp.max_depth = ctx->params.max_depth;
    if (sp.n_pix * bp.n_sets >= 0xFFFFFFFFull) return fail(-1, "tile too large for the bucket work queue");
    bp.n_items = (uint32_t)(sp.n_pix * bp.n_sets);
    for (uint32_t b = 0; b < ctx->n_buckets; b += 1)
    {
        bp.pixels[b] = ctx->buckets.pixels[b] + pix0 * (S + 1);
        bp.avgs[b] = ctx->buckets.avgs[b] + pix0 * S;
        bp.vars[b] = ctx->buckets.vars[b] + pix0 * S;
    }
    const uint64_t *records = ctx->d_records, *headers = ctx->d_headers;
    unsigned long long *queue = ctx->d_counters + DRT_NUM_COUNTERS + 3;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)bp.n_items + BUCKET_WAVES - 1) / BUCKET_WAVES, (uint64_t)ctx->buckets.grid_cap);
    void *args[] = {&ctx->dsc, &bp, &records, &headers, &queue};
    HIP_TRY(hipLaunchKernel(bucket_kernel(ctx->n_buckets, ctx->spds_in_lds), dim3(grid), dim3(BUCKET_BLOCK), args, depth_lds_bytes(ctx), ctx->stream));
    return 0;
}

/* The lobe pass of one kernel pair (lobes bound): drt_lobe_kernel over the pair's pixels and samples, behind its shade kernel. Its
 * queue is the cut pass's word, +3 of the pair's work words: of cuts, a sensor, buckets and lobes only one is ever bound. */
template <int NF>
static const void *lobe_kernel(bool lds) { return lds ? (const void *)drt_lobe_kernel<NF, true> : (const void *)drt_lobe_kernel<NF, false>; }
static const void *lobe_kernel(uint32_t n, bool lds)
{
    switch (n)
    {
        case 1: return lobe_kernel<1>(lds);
        case 2: return lobe_kernel<2>(lds);
        case 3: return lobe_kernel<3>(lds);
        case 4: return lobe_kernel<4>(lds);
        case 5: return lobe_kernel<5>(lds);
        case 6: return lobe_kernel<6>(lds);
        case 7: return lobe_kernel<7>(lds);
        default: return lobe_kernel<8>(lds);
    }
}

/* a map row as the kernel takes it: byte f is the film of function f */
static uint64_t lobe_row(const uint8_t *row)
{
    uint64_t w = 0;
    for (uint32_t f = 0; f < (uint32_t)DRT_NUM_BDSFS; f += 1) w |= (uint64_t)row[f] << (8 * f);
    return w;
}

static int launch_lobes(drt_context *ctx, const ShadeParams &sp, uint64_t pix0)
{
    const size_t S = ctx->dsc.S;
    LobeParams lp{};
    lp.n_pix = sp.n_pix;
    lp.n_samples = sp.n_samples;
    lp.first_sample = sp.first_sample;
    lp.vertex_words = sp.vertex_words;
    lp.block_words = sp.block_words;
    lp.n_lights = sp.n_lights;
    lp.batch = sp.batch;
    lp.overflow = sp.overflow;
    lp.n_sets = (uint32_t)((S + 63) / 64);
    lp.max_depth = ctx->params.max_depth;
    lp.emission = ctx->lobe_map.emission;
    lp.direct = lobe_row(ctx->lobe_map.direct);
    lp.indirect = lobe_row(ctx->lobe_map.indirect);
    if (sp.n_pix * lp.n_sets >= 0xFFFFFFFFull) return fail(-1, "tile too large for the lobe work queue");
    lp.n_items = (uint32_t)(sp.n_pix * lp.n_sets);
    for (uint32_t c = 0; c < ctx->n_lobes; c += 1)
    {
        lp.pixels[c] = ctx->lobes.pixels[c] + pix0 * (S + 1);
        lp.avgs[c] = ctx->lobes.avgs[c] + pix0 * S;
        lp.vars[c] = ctx->lobes.vars[c] + pix0 * S;
    }
    const uint64_t *records = ctx->d_records, *headers = ctx->d_headers;
    unsigned long long *queue = ctx->d_counters + DRT_NUM_COUNTERS + 3;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)lp.n_items + LOBE_WAVES - 1) / LOBE_WAVES, (uint64_t)ctx->lobes.grid_cap);
    void *args[] = {&ctx->dsc, &lp, &records, &headers, &queue};
    HIP_TRY(hipLaunchKernel(lobe_kernel(ctx->n_lobes, ctx->spds_in_lds), dim3(grid), dim3(LOBE_BLOCK), args, depth_lds_bytes(ctx), ctx->stream));
    return 0;
}

static int launch_sensor(drt_context *ctx, const ShadeParams &sp, uint64_t pix0)
{
    const size_t S = ctx->dsc.S, n = ctx->n_sensor;
    SensorParams np{};
    np.n_pix = sp.n_pix;
    np.n_samples = sp.n_samples;
    np.first_sample = sp.first_sample;
    np.vertex_words = sp.vertex_words;
    np.block_words = sp.block_words;
    np.n_lights = sp.n_lights;
    np.batch = sp.batch;
    np.overflow = sp.overflow;
    np.n_sets = (uint32_t)((S + 63) / 64);
    np.max_depth = ctx->params.max_depth;
    np.n_channels = ctx->n_sensor;
    if (sp.n_pix >= 0xFFFFFFFFull) return fail(-1, "tile too large for the sensor work queue");
    np.n_items = (uint32_t)sp.n_pix;
    np.curves = ctx->sensor.curves;
    np.pixels = ctx->sensor.pixels + pix0 * (n + 1);
    np.avgs = ctx->sensor.avgs + pix0 * n;
    np.vars = ctx->sensor.vars + pix0 * n;
    const uint64_t *records = ctx->d_records, *headers = ctx->d_headers;
    unsigned long long *queue = ctx->d_counters + DRT_NUM_COUNTERS + 3;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((sp.n_pix + SENSOR_WAVES - 1) / SENSOR_WAVES, (uint64_t)ctx->sensor.grid_cap);
    void *args[] = {&ctx->dsc, &np, &records, &headers, &queue};
    HIP_TRY(hipLaunchKernel(sensor_kernel(ctx->sensor.spds_in_lds), dim3(grid), dim3(SENSOR_BLOCK), args,
                            sensor_lds_bytes(ctx, ctx->n_sensor, ctx->sensor.spds_in_lds), ctx->stream));
    return 0;
}

template <int NSETS, bool XYZ>
static int shade_occupancy_mode(drt_context *ctx, int *per_cu)
{
    /* (the DARK instantiations have the same registers and LDS) */
    /* (a closed context's adaptive rounds launch the general LIST instantiation on the same grid cap, with its own LDS size: the closed
     * kernel is bound at five waves, the general one at four, so a workgroup in five of such a round only queues behind the
     * persistent ones and finds the work gone) */
#if DRT_SHADE_CLOSED_LDS_HEADERS
    if (NSETS == 1 && !XYZ && shade_closed_lds(ctx))
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, drt_shade_kernel_closed_lds<true>, SHADE_BLOCK, ctx->shade_lds_closed));
    else
#endif
    if (NSETS == 1 && !XYZ && shade_closed(ctx))
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, drt_shade_kernel_closed<true>, SHADE_BLOCK, ctx->shade_lds));
    else if (NSETS == 1 && shade_simple(ctx))
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, drt_shade_kernel<NSETS, true, XYZ, true, (NSETS == 1)>, SHADE_BLOCK, ctx->shade_lds));
    else if (ctx->spds_in_lds)
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, drt_shade_kernel<NSETS, true, XYZ, true>, SHADE_BLOCK, ctx->shade_lds));
    else
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, drt_shade_kernel<NSETS, false, XYZ, true>, SHADE_BLOCK, ctx->shade_lds));
    return 0;
}

template <int NSETS>
static int shade_occupancy(drt_context *ctx, int *per_cu)
{
    return ctx->xyz_mode ? shade_occupancy_mode<NSETS, true>(ctx, per_cu) : shade_occupancy_mode<NSETS, false>(ctx, per_cu);
}

extern "C" const char *drt_last_error(void) { return g_last_error.c_str(); }

/* Host only (no HIP call): builds the hierarchy build_device_scene() would build and reports its shape. */
extern "C" int drt_bvh_stats(const drt_scene *scene, uint32_t *nodes, uint32_t *leaf_surfaces, uint32_t *depth, uint32_t *stack_entries)
{
    g_last_error.clear();
    if (!scene) return fail(-1, "null argument");
    BvhBuilder bb;
    bb.build(scene, 0.0);
    if (nodes) *nodes = (uint32_t)bb.nodes.size();
    if (leaf_surfaces) *leaf_surfaces = (uint32_t)bb.order.size();
    if (depth) *depth = (uint32_t)bb.max_depth;
    if (stack_entries) *stack_entries = BVH_STACK;
    return 0;
}

extern "C" int drt_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(-1, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

/* bytes of the first film buffer: sum+filter rows, or the XYZ accumulators */
static size_t pixels_bytes(const drt_context *ctx)
{
    return (size_t)ctx->n_pix * (ctx->xyz_mode ? (size_t)XYZ_FILM_WORDS : (size_t)ctx->dsc.S + 1) * 8;
}

static int enqueue_trace(drt_context *ctx, const TraceTile &tile, const PairSpan &span);

/* waves of the trace-stage kernel that takes record blocks, for a launch of n_paths */
static uint64_t trace_waves(const drt_context *ctx, uint64_t n_paths)
{
    const uint64_t cap = (uint64_t)(ctx->bvh_pipeline ? ctx->bounce_grid_cap : ctx->trace_grid_cap);
    return std::min<uint64_t>(cap, (n_paths + TRACE_BLOCK - 1) / TRACE_BLOCK) * (TRACE_BLOCK / 64);
}
/* blocks that are enough for ANY launch of n_paths: every path max_depth vertices; fewer than 64 blocks of every POOL_CHUNK
 * stay unused when a wave moves on to a new chunk, every wave ends on a part-used one, and its lanes on a spare (or two) each */
static uint64_t blocks_worst_case(const drt_context *ctx, uint64_t n_paths)
{
    return (uint64_t)((double)n_paths * ctx->worst_blocks_per_path * (1.0 + 64.0 / POOL_CHUNK)) + trace_waves(ctx, n_paths) * (POOL_CHUNK + 2 * 64) + 1;
}

/* ray origins that are not on a surface are on the camera: its aperture and its film */
static double camera_reach(const drt_camera *camera)
{
    double reach = 0.0;
    for (int k = 0; k < 3; k += 1)
    {
        const double a = camera->aperture_position[k], f = camera->film_bottom_left[k];
        reach = std::max(reach, std::fabs(a) + 2.0 * std::fabs(f - a) + std::fabs(camera->aperture_radius));
    }
    return reach;
}

static void set_device_camera(drt_context *ctx, const drt_camera *camera)
{
    DevCamera &c = ctx->dcam;
    c.forward = hv(camera->forward); c.right = hv(camera->right); c.up = hv(camera->up);
    c.aperture_position = hv(camera->aperture_position); c.film_bottom_left = hv(camera->film_bottom_left);
    c.aperture_radius = camera->aperture_radius; c.focal_depth = camera->focal_depth;
    c.pixel_width = camera->pixel_width; c.pixel_height = camera->pixel_height;
    ctx->h_camera = *camera;
    ctx->win_dirty = true;
}

/* The live window of the context as it stands: from the host's surfaces and camera. After a device-mode surface update the host does
 * not know the bounds: the whole tile, until a host-mode update (or a read-back) makes h_surfaces current again. */
static LiveWindow live_window_of(const drt_surface *surfaces, size_t n_surf, const drt_material &escape, const drt_camera &camera, const drt_params &params)
{
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    bool any = false;
    for (size_t i = 0; i < n_surf; i += 1)
    {
        if (surfaces[i].type != DRT_GEO_SPHERE && surfaces[i].type != DRT_GEO_PLANE) continue; /* points are never intersected */
        double l[3], h[3];
        prim_bounds(surfaces[i], l, h);
        for (int k = 0; k < 3; k += 1)
        {
            if (!(l[k] <= h[k])) return live_window_whole(params); /* a NaN coordinate */
            lo[k] = std::min(lo[k], l[k]);
            hi[k] = std::max(hi[k], h[k]);
        }
        any = true;
    }
    const bool escape_dark = escape.is_black_body != 0u && escape.is_emissive == 0u;
    if (!any) return live_window_whole(params); /* nothing to bound: the rule does not apply */
    return live_window_rule(lo, hi, camera, params, escape_dark);
}

static void window_refresh(drt_context *ctx)
{
    if (!ctx->win_dirty) return;
    const drt_params &p = ctx->params;
    ctx->win = live_window_whole(p);
    if (ctx->win_allowed && !ctx->h_stale && ctx->dsc.escape_mat < ctx->ft_mats.size())
        ctx->win = live_window_of(ctx->h_surfaces.data(), ctx->h_surfaces.size(), ctx->ft_mats[ctx->dsc.escape_mat], ctx->h_camera, p);
    const LiveWindow &w = ctx->win;
    if (w.x_lo >= w.x_hi || w.y_lo >= w.y_hi) ctx->wx0 = ctx->wx1 = ctx->wy0 = ctx->wy1 = 0;
    else
    {
        ctx->wx0 = w.x_lo - p.x0;
        ctx->wx1 = w.x_hi - p.x0;
        /* tile row j is image row y0 + j row_stride */
        ctx->wy0 = (w.y_lo - p.y0 + p.row_stride - 1) / p.row_stride;
        ctx->wy1 = std::min<uint32_t>(p.tile_h, (w.y_hi - p.y0 + p.row_stride - 1) / p.row_stride);
        if (ctx->wy0 >= ctx->wy1) ctx->wx0 = ctx->wx1 = ctx->wy0 = ctx->wy1 = 0;
    }
    ctx->win_part = !w.whole && !(ctx->wx0 == 0 && ctx->wx1 == p.tile_w && ctx->wy0 == 0 && ctx->wy1 == p.tile_h);
    ctx->win_dirty = false;
}

/* whether dense pairs of this context go out windowed now */
static bool window_in_use(drt_context *ctx)
{
    window_refresh(ctx);
    return ctx->win_part && !(ctx->params.flags & DRT_FLAG_RECORD_HITS) && !ctx->rays_bound && ctx->n_cuts == 0 && ctx->n_sensor == 0 && ctx->n_buckets == 0 && ctx->n_lobes == 0;
}

static int create_impl(drt_context *ctx, const drt_scene *scene, const drt_camera *camera, const drt_params *params)
{
    if (!scene || !camera || !params) return fail(-1, "null argument");
    if (params->tile_w == 0 || params->tile_h == 0 || params->max_depth == 0) return fail(-1, "empty tile or zero depth");
    if (params->mode != DRT_MODE_SPECTRAL && params->mode != DRT_MODE_XYZ) return fail(-1, "unknown film mode %u", params->mode);
    ctx->xyz_mode = params->mode == DRT_MODE_XYZ;
    if ((uint64_t)params->x0 + params->tile_w > params->width || (uint64_t)params->y0 + (uint64_t)(params->tile_h - 1) * (params->row_stride ? params->row_stride : 1) >= params->height)
        return fail(-1, "tile does not fit the %ux%u image", params->width, params->height);
    ctx->params = *params;
    if (ctx->params.row_stride == 0) ctx->params.row_stride = 1;
    ctx->device = params->device;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->own_stream.create(hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    const double reach = camera_reach(camera);
    int rc = build_device_scene(ctx, scene, reach);
    if (rc) return rc;
    ctx->cam_reach = reach;
    ctx->h_surfaces.assign(scene->surfaces, scene->surfaces + scene->num_surfaces);
    ctx->ft_mats.assign(scene->materials, scene->materials + scene->num_materials);
    ctx->ft_n_spd = scene->num_spds;
    ctx->ft_S = scene->num_wavelengths;
    ctx->ft_spds.assign(scene->spds, scene->spds + (size_t)scene->num_spds * scene->num_wavelengths);
    if (const char *e = getenv("DRT_NO_LIVE_WINDOW")) ctx->win_allowed = atoi(e) == 0; /* A/B switch of the parity tests: same film either way */
    if (ctx->xyz_mode)
    {
        /* the XYZ film adds observer row x spectral sum x row per pair: +0 for a pair worth +0 only where the observer's rows are finite */
        const uint32_t rows[4] = {scene->cmf_rw, scene->cmf_x, scene->cmf_y, scene->cmf_z};
        for (int k = 0; k < 4; k += 1)
            for (uint32_t i = 0; i < scene->num_wavelengths; i += 1)
                if (!std::isfinite(scene->spds[(size_t)rows[k] * scene->num_wavelengths + i])) ctx->win_allowed = false;
    }

    set_device_camera(ctx, camera);

    const uint32_t S = scene->num_wavelengths;
    ctx->n_pix = (uint64_t)params->tile_w * params->tile_h;
    /* vertex record stride: fixed part + one block per light, rounded up to a power of two (>= 16 words) so a
     * vertex never straddles the shade kernel's 64-word prefetch registers */
    ctx->vertex_words = 16;
    while (ctx->vertex_words < REC_VERTEX_WORDS + REC_LIGHT_WORDS * ctx->dsc.n_lights) ctx->vertex_words *= 2;
    ctx->vertex_shift = 0;
    while ((1u << ctx->vertex_shift) < ctx->vertex_words) ctx->vertex_shift += 1;
    ctx->block_words = REC_BLOCK_VERTICES * ctx->vertex_words;
    /* a path of max_depth vertices: a block per four, plus the table block once the header's three are used up */
    const uint32_t deepest = (params->max_depth + REC_BLOCK_VERTICES - 1) / REC_BLOCK_VERTICES;
    ctx->worst_blocks_per_path = deepest + (deepest > REC_HEADER_BLOCKS ? 1u : 0u);
    if (deepest > REC_HEADER_BLOCKS + 2 * ctx->block_words)
        return fail(-2, "max_depth %u: a path's table block holds %u blocks beyond the header's %d", params->max_depth, 2 * ctx->block_words, REC_HEADER_BLOCKS);
    if (ctx->dsc.n_spd >= 0xFFFFu) return fail(-2, "too many SPDs for the 16-bit record indices");
    if (S > 64 * SHADE_MAX_SETS) return fail(-2, "more than %d wavelengths", 64 * SHADE_MAX_SETS);
    {
        uint32_t sets = 0, tf = 0, tc = 0;
        shade_sets(S, &sets, &tf, &tc);
        ctx->tail_count = tc;
    }
    /* scenes behind the hierarchy: camera rays walk it a wave at a time, the rest of each path runs from a queue (drt_bvh_kernels.h) */
    ctx->bvh_pipeline = !ctx->scene_in_lds;

    HIP_TRY(ctx->own_pixels.need(pixels_bytes(ctx) / 8));
    if (!ctx->xyz_mode)
    {
        HIP_TRY(ctx->own_avgs.need((size_t)ctx->n_pix * S));
        HIP_TRY(ctx->own_vars.need((size_t)ctx->n_pix * S));
    }
    ctx->d_pixels = ctx->own_pixels;
    ctx->d_avgs = ctx->own_avgs;
    ctx->d_vars = ctx->own_vars;
    ctx->own_film = true;
    HIP_TRY(hipMemsetAsync(ctx->d_pixels, 0, pixels_bytes(ctx), ctx->stream));
    if (ctx->d_avgs) HIP_TRY(hipMemsetAsync(ctx->d_avgs, 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
    if (ctx->d_vars) HIP_TRY(hipMemsetAsync(ctx->d_vars, 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
    HIP_TRY(ctx->d_counters.need(DRT_COUNTER_WORDS));
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, DRT_COUNTER_WORDS * sizeof(unsigned long long), ctx->stream));

    /* persistent trace grid: as many workgroups as the chip keeps resident */
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    int per_cu = 0;
    if (ctx->scene_in_lds && ctx->trace_tail) /* the instantiation that will be launched: its registers and LDS decide the grid */
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, drt_trace_direct_kernel<true, true>, TRACE_BLOCK, ctx->trace_lds));
    else if (ctx->scene_in_lds)
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, drt_trace_direct_kernel<true, false>, TRACE_BLOCK, ctx->trace_lds));
    /* The ray stash (drt_trace_kernel, 5 KB of LDS a wave): taken only where the block with it still is a plain 64 KB block and the
     * CU keeps as many of them as it keeps of the direct form; DRT_NO_RAY_STASH=1 is the A/B switch. scene_in_lds and the tail rule
     * do not count it. */
    ctx->trace_stash = false;
    if (ctx->scene_in_lds && !(getenv("DRT_NO_RAY_STASH") && atoi(getenv("DRT_NO_RAY_STASH")) != 0) && ctx->trace_lds + TRACE_STASH_BYTES <= 64 * 1024)
    {
        int with = 0;
        if (ctx->trace_tail) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&with, drt_trace_kernel<true, true>, TRACE_BLOCK, ctx->trace_lds + TRACE_STASH_BYTES));
        else HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&with, drt_trace_kernel<true, false>, TRACE_BLOCK, ctx->trace_lds + TRACE_STASH_BYTES));
        ctx->trace_stash = with >= 1 && with >= per_cu;
    }
    if (per_cu < 1) per_cu = 1;
    if (const char *e = getenv("DRT_TRACE_BLOCKS_PER_CU")) per_cu = std::max(1, atoi(e)); /* tuning knob */
    ctx->trace_grid_cap = prop.multiProcessorCount * per_cu;
    ctx->ray_grid_cap = prop.multiProcessorCount * 4; /* the ray-query kernels loop over ray blocks: a few workgroups per CU */
    if (const char *e = getenv("DRT_RAY_CHUNK")) /* test knob: host-mode ray queries in chunks this small */
        ctx->ray_chunk = std::max<uint64_t>(1, std::min<uint64_t>(RAY_STAGING_RAYS, strtoull(e, nullptr, 0)));
    if (ctx->bvh_pipeline)
    {
        int p_cu = 0, b_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p_cu, drt_primary_kernel<false>, PRIMARY_BLOCK, 0));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b_cu, drt_bounce_kernel<false>, BOUNCE_BLOCK, 0));
        if (const char *e = getenv("DRT_TRACE_BLOCKS_PER_CU")) b_cu = std::max(1, atoi(e));
        ctx->primary_grid_cap = prop.multiProcessorCount * std::max(1, p_cu);
        ctx->bounce_grid_cap = prop.multiProcessorCount * std::max(1, b_cu);
    }
    /* shade kernel LDS: SPD tables + two record buffers per wave */
    /* (drt_shade_lds_rule.h) a wave's own region: two record slots in the main pass (the coefficient words of plastic vertices are read
     * back from them), a window of headers in the tail pass; the closed instantiation's: one slot and the window's headers */
    const ShadeLdsPlan lds_general = shade_lds_plan(ctx->dsc.n_spd, S, ctx->spds_in_lds, SHADE_WAVES, SHADE_WAVE_LDS_WORDS_FOR(false), DRT_SHADE_WAVES_PER_SIMD);
    const ShadeLdsPlan lds_closed = shade_lds_plan(ctx->dsc.n_spd, S, ctx->spds_in_lds, SHADE_WAVES, SHADE_WAVE_LDS_WORDS_FOR(true), DRT_SHADE_WAVES_CLOSED_LDS);
    ctx->shade_lds = lds_general.group_bytes;
    ctx->shade_lds_closed = lds_closed.group_bytes;
    /* the form with headers in LDS is there for its fifth wave: where five workgroups do not fit beside the table, the closed kernel
     * with the headers in registers runs, as it does with DRT_NO_CLOSED_LDS=1 (the A/B of the two from one library) */
    ctx->closed_lds = lds_closed.groups >= DRT_SHADE_WAVES_CLOSED_LDS * SHADE_SIMDS_PER_CU / SHADE_WAVES && getenv("DRT_NO_CLOSED_LDS") == nullptr;
    /* Six waves: every workgroup holds the table, so a sixth workgroup of four waves never fits beside a table of 38 rows -- three
     * workgroups of eight waves with one table each do. The runtime is asked, and the form runs only where it answers three (asked
     * below, once the context's instantiation is known); DRT_CLOSED_WAVES=5 (or 4) keeps the five-wave kernel: the A/B from one library. */
    static_assert(SHADE_WAVES_CLOSED_LDS6 == SHADE_LDS_SIX_BLOCK_WAVES && DRT_SHADE_WAVES_CLOSED_LDS6 == SHADE_LDS_SIX_WAVES_PER_SIMD, "the rule's shape is the kernel's");
    const ShadeLdsPlan lds_closed6 = shade_lds_plan_six(ctx->dsc.n_spd, S, ctx->spds_in_lds, SHADE_WAVE_LDS_WORDS_FOR(true));
    ctx->shade_lds_closed6 = lds_closed6.group_bytes;
    const uint32_t groups6 = SHADE_LDS_SIX_GROUPS;
    int closed_waves_asked = DRT_SHADE_WAVES_CLOSED_LDS6;
    if (const char *e = getenv("DRT_CLOSED_WAVES")) closed_waves_asked = atoi(e);
    int s_per_cu = 0;
    shade_sets(S, &ctx->shade_sets, &ctx->tail_first, &ctx->tail_count);
    switch (ctx->shade_sets)
    {
        case 1: rc = shade_occupancy<1>(ctx, &s_per_cu); break;
        case 2: rc = shade_occupancy<2>(ctx, &s_per_cu); break;
        case 3: rc = shade_occupancy<3>(ctx, &s_per_cu); break;
        default: rc = shade_occupancy<4>(ctx, &s_per_cu); break;
    }
    if (rc) return rc;
    const int s_query = s_per_cu; /* what the runtime's occupancy query said */
    /* the closed kernel's grid never counts on more resident workgroups than the LDS rule allows (its register bound asks for one
     * more than the other instantiations': that one must also fit) */
    if (shade_closed_lds(ctx)) s_per_cu = std::min(s_per_cu, (int)lds_closed.groups);
    if (s_per_cu < 1) s_per_cu = 1;
    int s6_query = -1; /* the query's answer for the six-wave kernel (-1: not asked) */
#if DRT_SHADE_CLOSED_LDS_HEADERS
    if (shade_closed_lds(ctx) && closed_waves_asked >= DRT_SHADE_WAVES_CLOSED_LDS6 && shade_lds_six_fits(lds_closed6))
    {
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&s6_query, drt_shade_kernel_closed_lds6<true>, SHADE_BLOCK_CLOSED_LDS6, ctx->shade_lds_closed6));
        ctx->closed_lds6 = s6_query == (int)groups6; /* (more cannot be: the kernel's register bound; fewer: five waves of the other form are better) */
    }
#endif
    ctx->shade_grid_cap6 = prop.multiProcessorCount * (int)groups6;
    if (const char *e = getenv("DRT_SHADE_BLOCKS_PER_CU")) ctx->shade_grid_cap6 = prop.multiProcessorCount * std::min((int)groups6, std::max(1, atoi(e)));
    if (const char *e = getenv("DRT_SHADE_BLOCKS_PER_CU")) s_per_cu = std::max(1, atoi(e)); /* tuning knob */
    ctx->shade_grid_cap = prop.multiProcessorCount * s_per_cu;
    /* Both grids are persistent and fill every wave slot of the chip, so a kernel of another stream -- a collective's,
     * a copy's -- starts only when one of them ends. DRT_RESERVE_BLOCKS=n leaves n workgroup slots free for such
     * company (bench.py sets it when a gather runs behind the rendering). */
    if (const char *e = getenv("DRT_RESERVE_BLOCKS"))
    {
        int n = std::max(0, atoi(e));
        ctx->trace_grid_cap = std::max(1, ctx->trace_grid_cap - n);
        ctx->shade_grid_cap = std::max(1, ctx->shade_grid_cap - n);
        ctx->shade_grid_cap6 = std::max(1, ctx->shade_grid_cap6 - n);
    }
    if (const char *e = getenv("DRT_TRACE_CHUNK")) ctx->trace_chunk_override = (uint32_t)std::min(1 << 20, std::max(64, atoi(e) / 64 * 64));
    if (const char *e = getenv("DRT_TAIL_PERIOD")) ctx->shade_overrides.tail_period = (uint32_t)std::max(0, atoi(e));
    if (const char *e = getenv("DRT_SHADE_SUBS")) ctx->shade_overrides.subs = (uint32_t)std::max(0, atoi(e));
    if (const char *e = getenv("DRT_SHADE_CHUNK")) ctx->shade_overrides.chunk = (uint32_t)atoi(e); /* (shade_queue clamps it) */
    if (const char *e = getenv("DRT_DEBUG_SHADE_MODE")) ctx->debug_shade_mode = (uint32_t)atoi(e);
    if (const char *e = getenv("DRT_DEBUG_TAIL_PHASE_A_OFF")) ctx->debug_tail_phase_a_off = atoi(e) != 0;
    /*
     * The record pool and the launch size. A launch of N paths needs about N * b blocks, b = blocks per path on THIS tile of
     * THIS scene (0.9 on the Cornell frame, where a worst-case path would take 4): b is measured here, once, on a sample of the
     * tile (every k-th row, one sample per pixel, traced into a small pool sized for the worst case), and the pool gets 1.2 b
     * per path, a quarter more for what the waves' chunks leave unused, and a margin for small launches -- so 64 M paths take
     * 28 GB instead of 68. If a launch runs out after all, its
     * shade kernel and everything queued behind it do nothing and the host renders those samples again in launches sized for the
     * worst case (redo_batches): slower, never wrong. Launch size: large launches are the efficient ones (their last round is
     * amortised: DESIGN.md, work queues); the default (batch_spp = 0, a one-shot job) follows the job announced in params->spp -- about
     * 32 kernel pairs, at least 16 GB of records, at most 64 M paths per launch. A larger pool would save launches (one pair per row
     * block of the one-shot call instead of two: kernels 179 -> 171 ms with 40 GB) but a process that starts right after another has
     * freed tens of GB waits for the driver to scrub them, 1-2 s per 40 GB (tools/r03_oneshot_blocks.sh): 16 GB stays.
     * Callers that keep a context across many frames pass DRT_BATCH_RESIDENT (below) or a batch_spp of their own.
     */
    const size_t block_bytes = (size_t)ctx->block_words * 8;
    const uint64_t npx = std::max<uint64_t>(ctx->n_pix, 1);
    const size_t per_path_fixed = REC_HEADER_WORDS * 8 + (size_t)ctx->tail_count * 8 * (ctx->tail_resume ? 2 : 1) + /* tail_stage, and tail_resume beside it */
                                  (ctx->bvh_pipeline ? sizeof(PrimaryHit) + sizeof(uint64_t) : 0);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    ctx->est_blocks_per_path = (double)ctx->worst_blocks_per_path;
    if (npx * (uint64_t)ctx->worst_blocks_per_path * block_bytes > (256ull << 20) && !getenv("DRT_POOL_WORST_CASE"))
    {
        /* the sample: tile rows 0, k, 2k, ... with k such that it holds about 128 k paths. Where dense pairs will go out windowed, the
         * rows and columns of the live window: its paths are the ones that take blocks (a path outside takes none), 2.5 times the
         * tile's average on the Cornell frame, in launches of 0.4 times the paths -- so b below stays blocks per TILE path, and the pool
         * serves windowed and whole-tile launches of the same samples alike */
        const bool win = window_in_use(ctx);
        const PairWindow pw = {win, ctx->wx0, ctx->wx1, ctx->wy0, ctx->wy1};
        const uint64_t live_px = win ? (uint64_t)(ctx->wx1 - ctx->wx0) * (ctx->wy1 - ctx->wy0) : npx;
        const TraceTile sample = pool_sample_tile(ctx->params, pw, pool_sample_step(live_px));
        const uint64_t n_sample = sample.n_pix;
        ctx->pool_blocks = blocks_worst_case(ctx, n_sample);
        HIP_TRY(ctx->d_records.need(ctx->pool_blocks * ctx->block_words));
        HIP_TRY(ctx->d_headers.need(n_sample * REC_HEADER_WORDS));
        if (ctx->bvh_pipeline)
        {
            HIP_TRY(ctx->d_primary.need(n_sample));
            HIP_TRY(ctx->d_queue.need(n_sample));
        }
        if ((rc = enqueue_trace(ctx, sample, PairSpan::whole_tile(ctx->params.first_sample, 1, 0)))) return rc;
        unsigned long long used = 0; /* blocks handed to paths (the cursor also counts the waves' part-used chunks) */
        HIP_TRY(hipMemcpyAsync(&used, ctx->d_counters + DRT_PAIR_COUNTERS + 5, sizeof(used), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->est_blocks_per_path = (double)used / (double)n_sample * ((double)live_px / (double)npx);
        {
            /* vertices per path on the sample: a scene whose paths average three vertices and more is a closed one -- hardly a pixel
             * stays dark there, and the shade kernel without the test for it is the faster one (config 3: 1767 against 1806-1837 ms) */
            unsigned long long cnt[3] = {0, 0, 0}; /* paths, scans, shaded vertices of the sample */
            HIP_TRY(hipMemcpy(cnt, ctx->d_counters + DRT_PAIR_COUNTERS, sizeof(cnt), hipMemcpyDeviceToHost));
            /* the sample is the live window's where dense pairs go out windowed: its own figure decides for those pairs (hardly a pixel
             * of the window stays dark), and the figure of the whole tile -- the paths outside the window have no vertex -- for every
             * pair that is not windowed, as it did before there was a window */
            if (cnt[0] > 0)
            {
                const double per_path = (double)cnt[2] / (double)cnt[0];
                ctx->dark_skip_win = per_path < 3.0;
                ctx->dark_skip = per_path * ((double)live_px / (double)npx) < 3.0;
            }
        }
        ctx->d_records.reset();
        ctx->d_headers.reset();
        ctx->d_primary.reset();
        ctx->d_queue.reset();
        HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, DRT_COUNTER_WORDS * sizeof(unsigned long long), ctx->stream)); /* the sample does not count */
        ctx->ev_used = 0;
        ctx->ev_paths.clear();
    }
    /* blocks a launch of n paths is given: 1.3 x the expectation, 8 sigma of a sum of n on top (a path's block count has a
     * standard deviation below 2), never less than one sample per pixel in the worst case (what redo_batches launches) */
    auto blocks_for = [&](uint64_t n_paths) -> uint64_t {
        const double want = 1.2 * ctx->est_blocks_per_path * (double)n_paths + 16.0 * std::sqrt((double)n_paths) + 4096.0;
        const uint64_t expect = (uint64_t)(want * (1.0 + 64.0 / POOL_CHUNK)) + trace_waves(ctx, n_paths) * (POOL_CHUNK + 2 * 64) + 1; /* + the lanes' spares */
        return std::max<uint64_t>(std::min<uint64_t>(expect, blocks_worst_case(ctx, n_paths)), blocks_worst_case(ctx, npx));
    };
    uint32_t batch = params->batch_spp;
    if (batch == DRT_BATCH_RESIDENT)
    {
        /* a context kept across many frames: up to 256 M paths per kernel pair -- every launch ends on a partly idle chip (work
         * queues), and 288 GB of HBM hold the 116 GB of records that takes on the Cornell frame: 1024^2 x 256 spp in one pair instead of
         * four, 1525 -> 1568 Mpaths/s (the loop below halves the launch until its records fit half of what is free) -- but never fewer
         * than 16 samples per pixel and launch, because the film is read and written once per launch: 3328 bytes per pixel, which at
         * 4 samples a launch (the 4096^2 frame of config 5) was a third of the frame */
        const uint64_t resident_paths = getenv("DRT_RESIDENT_PATHS_M") ? (uint64_t)std::max(1, atoi(getenv("DRT_RESIDENT_PATHS_M"))) << 20 : (256ull << 20);
        const uint64_t by_paths = std::max<uint64_t>(1, std::min<uint64_t>(DRT_DEFAULT_MAX_BATCH, resident_paths / npx));
        batch = (uint32_t)std::max<uint64_t>(by_paths, 16);
        if (params->spp) batch = std::min(batch, params->spp);
    }
    else if (batch == 0)
    {
        const double path_bytes = 1.2 * (1.0 + 64.0 / POOL_CHUNK) * ctx->est_blocks_per_path * (double)block_bytes + (double)per_path_fixed;
        uint64_t by_job = (std::max<uint32_t>(params->spp, 1) + 31) / 32;
        uint64_t by_floor = (uint64_t)((double)(16ull << 30) / (path_bytes * (double)npx));
        uint64_t cap = std::max<uint64_t>(1, std::min<uint64_t>(DRT_DEFAULT_MAX_BATCH, (64ull << 20) / npx));
        batch = (uint32_t)std::max<uint64_t>(1, std::min(std::max(by_job, by_floor), cap));
        if (params->spp) batch = std::min(batch, params->spp);
    }
    batch = std::min<uint32_t>(batch, 4096);
    const size_t film_bytes = ctx->xyz_mode ? (size_t)ctx->n_pix * XYZ_FILM_WORDS * 8 : (size_t)ctx->n_pix * (3 * (size_t)S + 1) * 8;
    (void)film_bytes; /* allocated above: free_b already excludes it */
    auto bytes_for = [&](uint32_t b) -> size_t { return blocks_for(npx * b) * block_bytes + (size_t)npx * b * per_path_fixed; };
    while (batch > 1 && bytes_for(batch) > free_b / 2) batch /= 2;
    if (bytes_for(batch) > free_b) return fail(-3, "not enough device memory: need %zu bytes", bytes_for(batch));
    ctx->batch_spp = batch;
    ctx->pool_blocks = blocks_for(npx * batch);
    if (const char *e = getenv("DRT_POOL_BLOCKS")) /* test knob: a pool this small (never below one worst-case sample per pixel) */
    {
        /* ... per pixel of what a dense pair launches: with the live window in use that is the window (a row of the tile at least), so
         * that the knob makes windowed pairs run out as it makes whole-tile ones; the first pair that is not windowed grows the pool
         * to the whole tile's floor (pool_floor) */
        const bool win = window_in_use(ctx); /* (works the window out where the pool sample above has not) */
        const uint64_t live = (uint64_t)(ctx->wx1 - ctx->wx0) * (ctx->wy1 - ctx->wy0);
        const uint64_t floor_px = win ? std::min<uint64_t>(npx, std::max<uint64_t>(live, params->tile_w)) : npx;
        ctx->pool_blocks = std::max<uint64_t>(blocks_worst_case(ctx, floor_px), std::min<uint64_t>(ctx->pool_blocks, strtoull(e, nullptr, 0)));
    }
    if (ctx->pool_blocks >= 0xFFFFFFF0ull) return fail(-3, "record pool of %llu blocks: block numbers are 32 bits", (unsigned long long)ctx->pool_blocks);
    HIP_TRY(ctx->d_records.need(ctx->pool_blocks * ctx->block_words));
    HIP_TRY(ctx->d_headers.need((size_t)npx * batch * REC_HEADER_WORDS));
    if (ctx->bvh_pipeline)
    {
        HIP_TRY(ctx->d_primary.need((size_t)npx * batch));
        HIP_TRY(ctx->d_queue.need((size_t)npx * batch));
    }
    if (ctx->tail_count) HIP_TRY(ctx->d_tail_stage.need((size_t)npx * batch * ctx->tail_count));
    if (ctx->tail_count && ctx->tail_resume) HIP_TRY(ctx->d_tail_resume.need((size_t)npx * batch * ctx->tail_count));
    if (const char *e = getenv("DRT_DARK_SKIP")) ctx->dark_skip = ctx->dark_skip_win = atoi(e) != 0; /* A/B switch of the parity tests: same film either way */
    if (getenv("DRT_VERBOSE"))
        fprintf(stderr, "drt: shade kernel %s; six waves: %s, occupancy query %d workgroups of %d lanes per CU, lds %zu (LDS rule: %u), grid cap %d\n",
                shade_closed_lds6(ctx) ? "drt_shade_kernel_closed_lds6" : shade_closed_lds(ctx) ? "drt_shade_kernel_closed_lds" : shade_closed(ctx) ? "drt_shade_kernel_closed" : "drt_shade_kernel",
                shade_closed_lds6(ctx) ? "chosen" : s6_query >= 0 ? "refused by the query" : "not asked", s6_query, SHADE_BLOCK_CLOSED_LDS6, ctx->shade_lds_closed6,
                lds_closed6.groups, ctx->shade_grid_cap6);
    if (getenv("DRT_VERBOSE"))
        fprintf(stderr, "drt: %d CUs, trace %d blocks/CU (lds %zu), shade %d blocks/CU (%s, occupancy query %d, lds %zu; LDS rule: general %u, closed %u of %zu bytes), batch %u, %.3f blocks/path measured (worst %u), pool %.2f GB\n",
                prop.multiProcessorCount, per_cu, ctx->trace_lds, s_per_cu, shade_closed_lds(ctx) ? "closed, headers in LDS" : shade_closed(ctx) ? "closed" : "general", s_query,
                shade_closed_lds(ctx) ? ctx->shade_lds_closed : ctx->shade_lds, lds_general.groups_by_lds, lds_closed.groups_by_lds, lds_closed.group_bytes,
                ctx->batch_spp, ctx->est_blocks_per_path,
                ctx->worst_blocks_per_path, (double)(ctx->pool_blocks * block_bytes) / 1e9);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" drt_context *drt_create(const drt_scene *scene, const drt_camera *camera, const drt_params *params)
{
    g_last_error.clear();
    drt_context *ctx = new drt_context();
    int rc = create_impl(ctx, scene, camera, params);
    if (rc != 0)
    {
        std::string keep = g_last_error;
        drt_destroy(ctx);
        (void)hipGetLastError();
        g_last_error = keep;
        return nullptr;
    }
    return ctx;
}

extern "C" void drt_destroy(drt_context *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
}

extern "C" int drt_bind_film(drt_context *ctx, void *d_pixels, void *d_avgs, void *d_vars)
{
    if (!ctx || !d_pixels || (!ctx->xyz_mode && (!d_avgs || !d_vars))) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->own_pixels.reset();
    ctx->own_avgs.reset();
    ctx->own_vars.reset();
    ctx->own_film = false;
    ctx->film_gen += 1;
    ctx->d_pixels = (double *)d_pixels;
    ctx->d_avgs = (double *)d_avgs;
    ctx->d_vars = (double *)d_vars;
    return 0;
}

extern "C" int drt_set_stream(drt_context *ctx, void *hip_stream)
{
    if (!ctx) return fail(-1, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return 0;
}

extern "C" int drt_synchronize(drt_context *ctx);

static int next_events(drt_context *ctx, hipEvent_t out[3])
{
    if (ctx->ev.size() < ctx->ev_used + 3) ctx->ev.resize(ctx->ev_used + 3);
    for (int k = 0; k < 3; k += 1) HIP_TRY(ctx->ev[ctx->ev_used + k].need());
    for (int k = 0; k < 3; k += 1) out[k] = ctx->ev[ctx->ev_used + k];
    ctx->ev_used += 3;
    return 0;
}

/* fold finished event triples into trace_ms / shade_ms (stream must be idle) */
static int collect_timings(drt_context *ctx)
{
    for (size_t k = 0; k + 3 <= ctx->ev_used; k += 3)
    {
        float a = 0.f, b = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, ctx->ev[k], ctx->ev[k + 1]));
        HIP_TRY(hipEventElapsedTime(&b, ctx->ev[k + 1], ctx->ev[k + 2]));
        ctx->trace_ms += a;
        ctx->shade_ms += b;
        const double paths = k / 3 < ctx->ev_paths.size() ? ctx->ev_paths[k / 3] : 0.0;
        if (paths > 0.0)
        {
            const double t = ((double)a + (double)b) * (double)ctx->n_pix / paths; /* one sample of every tile pixel at this pair's rate */
            if (ctx->timed_pairs == 0 || t < ctx->min_sample_ms) ctx->min_sample_ms = t;
            if (ctx->timed_pairs == 0 || t > ctx->max_sample_ms) ctx->max_sample_ms = t;
            ctx->timed_pairs += 1;
            ctx->avg_sample_ms += (t - ctx->avg_sample_ms) / (double)ctx->timed_pairs;
        }
    }
    ctx->ev_used = 0;
    ctx->ev_paths.clear();
    return 0;
}

/* after a kernel pair: if the pool did not run out, this pair is the last complete one; the pool's high-water mark */
__global__ void drt_mark_pair_kernel(unsigned long long *totals, unsigned long long seq)
{
    /* state[0] pool cursor of this pair, [1] overflow flag, [2] last complete pair, [3] peak of the cursor */
    unsigned long long *state = totals + DRT_NUM_COUNTERS + 4, *pair = totals + DRT_PAIR_COUNTERS;
    const bool complete = *(const uint32_t *)(state + 1) == 0u;
    if (complete) state[2] = seq;
    if (state[0] > state[3]) state[3] = state[0];
    for (int k = 0; k < DRT_NUM_COUNTERS; k += 1)
    {
        if (complete) totals[k] += pair[k]; /* an incomplete pair is rendered again: its paths are counted then */
        pair[k] = 0;
    }
}

static WindowParams window_params(const drt_context *ctx)
{
    WindowParams wp{};
    wp.tile_w = ctx->params.tile_w;
    wp.wx0 = ctx->wx0; wp.wx1 = ctx->wx1; wp.wy0 = ctx->wy0; wp.wy1 = ctx->wy1;
    wp.S = ctx->dsc.S;
    wp.xyz = ctx->xyz_mode ? 1u : 0u;
    wp.tail = ctx->tail_count ? 1u : 0u;
    wp.draws = ctx->params.pixel_scheme == DRT_FILM_SAMPLE_RANDOM ? 2u : 0u;
    return wp;
}

static PairWindow pair_window(const drt_context *ctx) { return {ctx->win_open, ctx->wx0, ctx->wx1, ctx->wy0, ctx->wy1}; }

/* While the window is open: the window's part of tile rows [row0, row0 + rows) (rows == 0: of the whole tile) into the staging film
 * (to_stage), or back. Dense pairs of those rows go in between. */
static int window_copy(drt_context *ctx, bool to_stage, uint32_t row0 = 0, uint32_t rows = 0)
{
    if (!ctx->win_open) return 0;
    WindowParams wp = window_params(ctx);
    const WindowRows r = window_rows(row0, rows, ctx->params.tile_h, pair_window(ctx));
    if (r.nothing) return 0;
    const uint64_t stage0 = r.stage0; /* the rows' first pixel in the staging film */
    wp.wy0 = r.lo; wp.wy1 = r.hi;
    const uint64_t pix = (uint64_t)(wp.wx1 - wp.wx0) * (r.hi - r.lo);
    double *const film[3] = {ctx->d_pixels, ctx->d_avgs, ctx->d_vars};
    const uint32_t words[3] = {ctx->xyz_mode ? (uint32_t)XYZ_FILM_WORDS : wp.S + 1u, wp.S, wp.S};
    for (int f = 0; f < (ctx->xyz_mode ? 1 : 3); f += 1)
    {
        const uint64_t n = pix * words[f];
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + WINDOW_BLOCK - 1) / WINDOW_BLOCK, 1u << 16);
        hipLaunchKernelGGL(drt_window_copy_kernel, dim3(grid), dim3(WINDOW_BLOCK), 0, ctx->stream, film[f], ctx->d_win_film[f] + stage0 * words[f], wp, words[f],
                           to_stage ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

/* Before the dense pairs of a render call: if they can use the live window, the pairs up to window_close are windowed ones, on the
 * staging film (window_copy moves the rows). It grows when the window has (after a camera move); that waits for the stream. */
static int window_open(drt_context *ctx)
{
    ctx->win_open = false;
    if (!window_in_use(ctx)) return 0;
    const uint64_t pix = (uint64_t)(ctx->wx1 - ctx->wx0) * (ctx->wy1 - ctx->wy0);
    if (pix > ctx->win_film_pix)
    {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        const size_t S = ctx->dsc.S;
        ctx->win_film_pix = 0;
        HIP_TRY(ctx->d_win_film[0].remake(pix * (ctx->xyz_mode ? (size_t)XYZ_FILM_WORDS : S + 1)));
        if (!ctx->xyz_mode)
        {
            HIP_TRY(ctx->d_win_film[1].remake(pix * S));
            HIP_TRY(ctx->d_win_film[2].remake(pix * S));
        }
        ctx->win_film_pix = pix;
    }
    ctx->win_open = true;
    return 0;
}

static void window_close(drt_context *ctx) { ctx->win_open = false; }

/* A pair over the whole tile, or over a pixel list, counts on a pool that holds one worst-case sample of every tile pixel (what
 * redo_batches launches). Only the DRT_POOL_BLOCKS test knob makes a pool smaller than that, sized for the window's pixels: the
 * first pair that is not windowed makes it the tile's. Waits for the stream: nothing in flight reads the records then. */
static int pool_floor(drt_context *ctx)
{
    const uint64_t floor_blocks = blocks_worst_case(ctx, ctx->n_pix);
    if (ctx->pool_blocks >= floor_blocks) return 0;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx->d_records.remake(floor_blocks * ctx->block_words));
    ctx->pool_blocks = floor_blocks;
    return 0;
}

/* behind a windowed pair's shade kernel: the pair's pixels outside the window (drt_window_fill_kernel) */
static int enqueue_window_fill(drt_context *ctx, uint32_t first_sample, uint32_t n, uint32_t row0, uint32_t rows)
{
    WindowParams wp = window_params(ctx);
    wp.row0 = row0; wp.rows = rows;
    wp.first_sample = first_sample; wp.n_samples = n;
    const uint64_t threads = (uint64_t)rows * wp.tile_w * (wp.xyz ? 7u : wp.S + 1u);
    const uint64_t grid = (threads + WINDOW_BLOCK - 1) / WINDOW_BLOCK;
    if (grid == 0) return 0;
    if (grid >= 0x7FFFFFFFull) return fail(-1, "tile too large for the live window's fill pass");
    hipLaunchKernelGGL(drt_window_fill_kernel, dim3((uint32_t)grid), dim3(WINDOW_BLOCK), 0, ctx->stream, ctx->d_pixels, ctx->d_avgs, ctx->d_vars, wp,
                       (const uint32_t *)(ctx->d_counters + DRT_NUM_COUNTERS + 5), ctx->d_counters + DRT_PAIR_COUNTERS);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* The trace stage of one kernel pair over samples [first_sample, first_sample + n) of every tile pixel: work queues and the
 * pool cursor reset, then drt_trace_kernel (scene in LDS) or drt_primary_kernel + drt_bounce_kernel (scene behind the hierarchy). */
static int enqueue_trace(drt_context *ctx, const TraceTile &tile, const PairSpan &span)
{
    const drt_params &p = ctx->params;
    const uint32_t *const list = span.list;
    TraceParams tp{};
    tp.width = p.width; tp.height = p.height; tp.x0 = tile.x0; tp.y0 = tile.y0;
    tp.tile_w = tile.tile_w; tp.tile_h = tile.tile_h; tp.row_stride = tile.row_stride;
    tp.first_sample = span.first_sample;
    tp.n_samples = span.n_samples;
    tp.max_depth = p.max_depth;
    tp.pixel_scheme = p.pixel_scheme;
    tp.record_hits = tile.record_hits;
    tp.seed = p.seed;
    tp.n_pix = tile.n_pix;
    tp.pixel_list = list;
    tp.sample_base = list ? ctx->d_counts : nullptr;
    tp.n_paths = tp.n_pix * span.n_samples;
    tp.vertex_words = ctx->vertex_words;
    tp.block_words = ctx->block_words;
    tp.hits_sample_offset = span.hits_sample_offset;
    tp.batch = tile.batch;
    tp.pool_blocks = (uint32_t)ctx->pool_blocks;
    tp.tail_stage = ctx->trace_tail ? ctx->d_tail_stage : nullptr;
    tp.tail_resume = tp.tail_stage ? ctx->d_tail_resume : nullptr;
    tp.spd_tail = ctx->d_spd_tail;
    tp.tail_count = ctx->tail_count;
    tp.n_spd = ctx->dsc.n_spd;
    unsigned long long *work = ctx->d_counters + DRT_NUM_COUNTERS;
    tp.pool_cursor = work + 4;
    tp.overflow = (uint32_t *)(work + 5);
    HIP_TRY(hipMemsetAsync(work, 0, 5 * sizeof(unsigned long long), ctx->stream)); /* trace + shade work queues, bounce queue length, spare, pool cursor */
    const uint32_t grid = trace_grid(tp.n_paths, TRACE_BLOCK, (uint32_t)(ctx->bvh_pipeline ? ctx->bounce_grid_cap : ctx->trace_grid_cap));
    tp.chunk = trace_chunk(tp.n_paths, grid, TRACE_BLOCK, ctx->bvh_pipeline, ctx->trace_chunk_override);
    /* a bound ray table: the same launches through the ray-mode entry points, the table behind their arguments */
    DevRayTable rt = ctx->rt;
    rt.t_offset = tile.t_offset;
    const bool rays = ctx->rays_bound;
    if (ctx->bvh_pipeline)
    {
        /* camera rays: a wave per 64 path ids; then the queued paths, one per lane */
        const uint64_t packets = (tp.n_paths + 63) / 64;
        const uint32_t pgrid = (uint32_t)std::min<uint64_t>((packets + PRIMARY_BLOCK / 64 - 1) / (PRIMARY_BLOCK / 64), (uint64_t)ctx->primary_grid_cap);
#define DRT_BVH_ARGS_P ctx->dsc, ctx->dcam, tp, ctx->d_headers, ctx->d_hits, ctx->d_counters + DRT_PAIR_COUNTERS, ctx->d_primary, ctx->d_queue, work + 2
#define DRT_BVH_ARGS_B ctx->dsc, ctx->dcam, tp, ctx->d_records, ctx->d_headers, ctx->d_hits, ctx->d_counters + DRT_PAIR_COUNTERS, work, ctx->d_primary, ctx->d_queue, work + 2
#define DRT_LAUNCH_BVH(LIST)                                                                                                              \
        if (rays) hipLaunchKernelGGL(drt_primary_rays_kernel<LIST>, dim3(pgrid), dim3(PRIMARY_BLOCK), 0, ctx->stream, DRT_BVH_ARGS_P, rt); \
        else hipLaunchKernelGGL(drt_primary_kernel<LIST>, dim3(pgrid), dim3(PRIMARY_BLOCK), 0, ctx->stream, DRT_BVH_ARGS_P);               \
        HIP_TRY(hipGetLastError());                                                                                                       \
        if (rays) hipLaunchKernelGGL(drt_bounce_rays_kernel<LIST>, dim3(grid), dim3(BOUNCE_BLOCK), 0, ctx->stream, DRT_BVH_ARGS_B, rt);    \
        else hipLaunchKernelGGL(drt_bounce_kernel<LIST>, dim3(grid), dim3(BOUNCE_BLOCK), 0, ctx->stream, DRT_BVH_ARGS_B)
        if (list) { DRT_LAUNCH_BVH(true); }
        else { DRT_LAUNCH_BVH(false); }
#undef DRT_LAUNCH_BVH
#undef DRT_BVH_ARGS_P
#undef DRT_BVH_ARGS_B
    }
    else
    {
#define DRT_TRACE_ARGS ctx->dsc, ctx->dcam, tp, ctx->d_records, ctx->d_headers, ctx->d_hits, ctx->d_counters + DRT_PAIR_COUNTERS, work
#define DRT_LAUNCH_TRACE(TAIL, LIST)                                                                                                                       \
        if (rays) hipLaunchKernelGGL((drt_trace_rays_kernel<true, TAIL, LIST>), dim3(grid), dim3(TRACE_BLOCK), ctx->trace_lds, ctx->stream, DRT_TRACE_ARGS, rt); \
        else if (ctx->trace_stash) hipLaunchKernelGGL((drt_trace_kernel<true, TAIL, LIST>), dim3(grid), dim3(TRACE_BLOCK), ctx->trace_lds + TRACE_STASH_BYTES, ctx->stream, DRT_TRACE_ARGS); \
        else hipLaunchKernelGGL((drt_trace_direct_kernel<true, TAIL, LIST>), dim3(grid), dim3(TRACE_BLOCK), ctx->trace_lds, ctx->stream, DRT_TRACE_ARGS)
        const bool tail = ctx->trace_tail && tp.tail_stage;
        if (list && tail) { DRT_LAUNCH_TRACE(true, true); }
        else if (list) { DRT_LAUNCH_TRACE(false, true); }
        else if (tail) { DRT_LAUNCH_TRACE(true, false); }
        else { DRT_LAUNCH_TRACE(false, false); }
#undef DRT_LAUNCH_TRACE
#undef DRT_TRACE_ARGS
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

/* One kernel pair: trace, shade + film, and the mark that tells the host whether the pair was complete. */
static int enqueue_pair(drt_context *ctx, const PairSpan &span)
{
    hipEvent_t ev[3];
    int rc = next_events(ctx, ev);
    if (rc) return rc;
    ctx->film_gen += 1;
    HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    /* A windowed pair (between window_open and window_close): the kernels' tile is the live window's part of the pair's rows, their
     * film the staging film; the pair's other pixels are drt_window_fill_kernel's, below. Nothing live in these rows: no kernels. */
    const PairGeometry g = pair_geometry(span, ctx->params.tile_w, ctx->params.tile_h, pair_window(ctx));
    if (!g.windowed && (rc = pool_floor(ctx))) return rc;
    if (!g.nothing && (rc = enqueue_trace(ctx, pair_trace_tile(ctx->params, ctx->n_pix, ctx->batch_spp, span, g), span))) return rc;
    HIP_TRY(hipEventRecord(ev[1], ctx->stream));

    unsigned long long *work = ctx->d_counters + DRT_NUM_COUNTERS;
    ShadeParams sp{};
    sp.n_pix = g.n_pix;
    sp.n_samples = span.n_samples;
    sp.first_sample = span.first_sample;
    sp.vertex_words = ctx->vertex_words;
    sp.vertex_shift = ctx->vertex_shift;
    sp.block_words = ctx->block_words;
    sp.overflow = (const uint32_t *)(work + 5);
    sp.n_lights = ctx->dsc.n_lights;
    sp.batch = span.stride ? span.stride : ctx->batch_spp;
    sp.tail_first = ctx->tail_first;
    sp.tail_count = ctx->tail_count;
    sp.tail_stage = ctx->d_tail_stage;
    sp.tail_resume = ctx->d_tail_resume;
    sp.light0_em_spd = ctx->light0_em_spd;
    sp.no_fixed_lists = ctx->no_fixed_lists ? 1u : 0u;
    sp.tail_staged = ((ctx->tail_all_staged && ctx->d_tail_stage) || ctx->debug_tail_phase_a_off) ? 1u : 0u;
    sp.pixel_list = span.list;
    sp.sample_base = span.list ? ctx->d_counts : nullptr;
    sp.mode = ctx->debug_shade_mode;
    sp.cmf_rw = ctx->cmf_rw; sp.cmf_x = ctx->cmf_x; sp.cmf_y = ctx->cmf_y; sp.cmf_z = ctx->cmf_z;
    const ShadeQueue q = shade_queue(g.n_pix, span.n_samples, ctx->tail_count, sp.tail_staged, shade_launch_grid_cap(ctx, span.list != nullptr),
                                     shade_launch_waves(ctx, span.list != nullptr), SHADE_PIXEL_CHUNK,
                                     ctx->shade_overrides);
    if (q.too_large) return fail(-1, "tile too large for the shade work queue");
    sp.chunk = q.chunk;
    sp.sub_pixels = q.sub_pixels;
    sp.items_per_group = q.items_per_group;
    sp.n_items = q.n_items;
    sp.tail_period_mains = q.tail_period_mains;
    const size_t S_ = ctx->dsc.S;
    const size_t film_words = ctx->xyz_mode ? (size_t)XYZ_FILM_WORDS : S_ + 1;
    double *const film[3] = {g.windowed ? ctx->d_win_film[0] + g.stage0 * film_words : ctx->d_pixels + g.pix0 * film_words,
                             g.windowed ? (ctx->xyz_mode ? nullptr : ctx->d_win_film[1] + g.stage0 * S_) : ctx->d_avgs ? ctx->d_avgs + g.pix0 * S_ : nullptr,
                             g.windowed ? (ctx->xyz_mode ? nullptr : ctx->d_win_film[2] + g.stage0 * S_) : ctx->d_vars ? ctx->d_vars + g.pix0 * S_ : nullptr};
    if (!g.nothing)
    {
        rc = launch_shade(ctx, q.grid, sp, film);
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
    }
    if (ctx->n_cuts && (rc = launch_depth_cuts(ctx, sp, g.pix0))) return rc;
    if (ctx->n_sensor && (rc = launch_sensor(ctx, sp, g.pix0))) return rc;
    if (ctx->n_buckets && (rc = launch_buckets(ctx, sp, g.pix0))) return rc;
    if (ctx->n_lobes && (rc = launch_lobes(ctx, sp, g.pix0))) return rc;
    if (g.windowed && (rc = enqueue_window_fill(ctx, span.first_sample, span.n_samples, g.t_row0, g.t_rows))) return rc;
    const uint64_t seq = ctx->next_seq++;
    hipLaunchKernelGGL(drt_mark_pair_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->d_counters, (unsigned long long)seq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[2], ctx->stream));
    ctx->ev_paths.resize(ctx->ev_used / 3, 0.0);
    ctx->ev_paths[ctx->ev_used / 3 - 1] = (double)g.counted_paths;
    ctx->inflight.push_back({span, seq});
    return 0;
}

/* The pool ran out in some kernel pair: that pair's shade kernel and every later kernel did nothing. Render those samples again,
 * in launches small enough for the worst case (every path max_depth vertices), synchronously. */
static int redo_batches(drt_context *ctx, uint64_t last_good_seq)
{
    std::vector<drt_context::Batch> todo;
    for (const auto &b : ctx->inflight) if (b.seq > last_good_seq) todo.push_back(b);
    ctx->inflight.clear();
    unsigned long long *work = ctx->d_counters + DRT_NUM_COUNTERS;
    HIP_TRY(hipMemsetAsync(work + 5, 0, sizeof(unsigned long long), ctx->stream)); /* the overflow flag */
    /* samples per launch that fit the pool whatever the paths do (one always does: the pool is never smaller, create_impl) */
    uint32_t safe = 1;
    while (safe < ctx->batch_spp && blocks_worst_case(ctx, ctx->n_pix * (uint64_t)(safe + 1)) <= ctx->pool_blocks) safe += 1;
    /* Dense pairs are replayed as windowed pairs where the context can use the live window (the pair that ran out and everything
     * behind it, fills included, did nothing; the staging film went back as the last complete pair left it). A render call that
     * synchronises does so before it has staged anything, so the film is whole here, whether the window is open already or not. */
    bool lists = false; /* (pixel-list pairs write the film itself: no staging film around them) */
    for (const auto &b : todo) lists = lists || b.span.list != nullptr;
    const bool was_open = ctx->win_open;
    int rc = 0;
    if (lists) window_close(ctx);
    else if (!was_open) rc = window_open(ctx);
    if (!rc) rc = window_copy(ctx, true);
    if (rc) { ctx->win_open = was_open; return rc; }
    for (const auto &b : todo)
    {
        ctx->redone_batches += 1;
        for (uint32_t done = 0; done < b.span.n_samples; done += safe)
        {
            /* (the hit log is indexed by sample offset within the caller's drt_render call: the span remembers its own) */
            rc = enqueue_pair(ctx, b.span.narrowed(done, std::min(safe, b.span.n_samples - done)));
            if (rc) break;
        }
        if (rc) break;
    }
    {
        const int rc_back = window_copy(ctx, false);
        if (!rc) rc = rc_back;
        ctx->win_open = was_open;
    }
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long st[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(st, work + 4, sizeof(st), hipMemcpyDeviceToHost));
    if ((uint32_t)st[1] != 0u) return fail(-6, "record pool exhausted in a launch sized for the worst case (%llu blocks)", (unsigned long long)ctx->pool_blocks);
    ctx->inflight.clear();
    return 0;
}

/* Samples [first_sample, first_sample + num_samples) of the tile in n_blocks row blocks, each with ALL the samples before the next
 * block starts, so that the film -- read and written once per pair, 3328 bytes a pixel -- is touched that much less often. Samples per
 * pair: row_block_fit, in pairs of equal size (drt_pair_rule.h); a block that runs out of records anyway is rendered again
 * (redo_batches). done[k], if asked for, is recorded behind block k. */
static int enqueue_blocks(drt_context *ctx, uint32_t first_sample, uint32_t num_samples, uint32_t n_blocks, std::vector<Event> *done)
{
    const uint32_t H = ctx->params.tile_h, W = ctx->params.tile_w;
    const uint32_t per = row_block_rows(H, n_blocks);
    const EqualSplit split = equal_split(num_samples, row_block_fit(num_samples, ctx->n_pix, ctx->batch_spp, per, W));
    for (uint32_t r0 = 0; r0 < H; r0 += per)
    {
        const uint32_t rows = std::min(per, H - r0);
        int rc = window_copy(ctx, true, r0, rows); /* (an open live window: the block's part of it, there and back around the block's pairs) */
        for (uint32_t i = 0, at = 0; i < split.n_pairs && !rc; at += split.size(i), i += 1)
            rc = enqueue_pair(ctx, PairSpan::row_block(first_sample + at, split.size(i), r0, rows));
        const int rc_back = window_copy(ctx, false, r0, rows);
        if (rc || rc_back) return rc ? rc : rc_back;
        if (done)
        {
            done->emplace_back();
            HIP_TRY(done->back().need(hipEventDisableTiming));
            HIP_TRY(hipEventRecord(done->back(), ctx->stream));
        }
    }
    return 0;
}

static int render_impl(drt_context *ctx, uint32_t first_sample, uint32_t num_samples);

extern "C" int drt_render(drt_context *ctx, uint32_t first_sample, uint32_t num_samples)
{
    if (!ctx) return fail(-1, "null context");
    if (ctx->adaptive_done) return fail(-7, "the film holds an adaptive render: drt_reset_film first");
    ctx->film_used = true;
    const int rc = render_impl(ctx, first_sample, num_samples);
    if (!rc && ctx->n_buckets) ctx->bk_samples += num_samples;
    return rc;
}

static int render_pairs(drt_context *ctx, uint32_t first_sample, uint32_t num_samples);

/* the call's dense pairs, between the live window's two film copies where the context can use it */
static int render_impl(drt_context *ctx, uint32_t first_sample, uint32_t num_samples)
{
    HIP_TRY(hipSetDevice(ctx->device));
    (void)hipGetLastError(); /* (as render_pairs: a stale error of an earlier, unrelated call) */
    int rc = window_open(ctx);
    if (rc) return rc;
    rc = render_pairs(ctx, first_sample, num_samples);
    window_close(ctx);
    return rc;
}

static int render_pairs(drt_context *ctx, uint32_t first_sample, uint32_t num_samples)
{
    HIP_TRY(hipSetDevice(ctx->device));
    (void)hipGetLastError(); /* drop a stale error of an earlier, unrelated call: launches below are checked against a clean slate */
    const drt_params &p = ctx->params;
    if (p.flags & DRT_FLAG_RECORD_HITS)
    {
        uint64_t need = ctx->n_pix * (uint64_t)num_samples;
        if (need > ctx->hits_capacity)
        {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx->d_hits.remake(std::max<uint64_t>(need, 1) * p.max_depth));
            ctx->hits_capacity = need;
        }
        ctx->hits_samples = num_samples;
    }
    /* keep the number of pending timing events bounded */
    if (ctx->ev_used >= 3 * 256)
    {
        int rc = drt_synchronize(ctx);
        if (rc) return rc;
    }
    /* Row blocks where row_block_count (drt_pair_rule.h) says they pay. Not with the hit log on, which is laid out by sample of the whole tile. */
    if (!(p.flags & DRT_FLAG_RECORD_HITS) && !getenv("DRT_NO_ROW_BLOCKS"))
    {
        const uint32_t n_blocks = row_block_count(num_samples, ctx->batch_spp, p.tile_h);
        if (n_blocks > 1) return enqueue_blocks(ctx, first_sample, num_samples, n_blocks, nullptr);
    }
    const EqualSplit split = equal_split(num_samples, ctx->batch_spp);
    int rc = window_copy(ctx, true);
    for (uint32_t i = 0, done = 0; i < split.n_pairs && !rc; done += split.size(i), i += 1)
        rc = enqueue_pair(ctx, PairSpan::whole_tile(first_sample + done, split.size(i), done));
    const int rc_back = window_copy(ctx, false);
    return rc ? rc : rc_back;
}

static int synchronize_impl(drt_context *ctx);

/* A device-mode update whose surfaces took the extent to 2^27 or beyond (the one condition the host cannot check before the call
 * returns) fails every synchronising call from then on, until a later update or drt_set_camera brings the extent back. */
extern "C" int drt_synchronize(drt_context *ctx)
{
    if (!ctx) return fail(-1, "null context");
    int rc = synchronize_impl(ctx);
    if (rc) return rc;
    if (ctx->upd_check)
    {
        unsigned long long word = 0;
        HIP_TRY(hipMemcpy(&word, ctx->d_upd_status + 1, sizeof(word), hipMemcpyDeviceToHost));
        ctx->upd_violation = word != 0ull;
        ctx->upd_check = false;
    }
    if (ctx->upd_violation)
        return fail(-2, "drt_update_surfaces: the updated surfaces' coordinates reach 2^27 or beyond, and the hierarchy's f32 box test holds up to 2^27: "
                        "what was rendered since is not held to the rule; update the surfaces again");
    return 0;
}

static int synchronize_impl(drt_context *ctx)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int rc = collect_timings(ctx);
    if (rc) return rc;
    if (!ctx->inflight.empty())
    {
        unsigned long long st[4] = {0, 0, 0, 0}; /* pool cursor, overflow flag, last complete pair, peak of the cursor */
        HIP_TRY(hipMemcpy(st, ctx->d_counters + DRT_NUM_COUNTERS + 4, sizeof(st), hipMemcpyDeviceToHost));
        ctx->pool_peak = std::max<uint64_t>(ctx->pool_peak, st[3]);
        if ((uint32_t)st[1] != 0u)
        {
            if ((rc = redo_batches(ctx, st[2]))) return rc;
            if ((rc = collect_timings(ctx))) return rc;
        }
        ctx->inflight.clear();
    }
    return 0;
}

extern "C" int drt_reset_film(drt_context *ctx)
{
    if (!ctx) return fail(-1, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = synchronize_impl(ctx); /* (not drt_synchronize: a film is reset before the update that mends a refused extent) */
    if (rc) return rc;
    const size_t S = ctx->dsc.S;
    HIP_TRY(hipMemsetAsync(ctx->d_pixels, 0, pixels_bytes(ctx), ctx->stream));
    if (ctx->d_avgs) HIP_TRY(hipMemsetAsync(ctx->d_avgs, 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
    if (ctx->d_vars) HIP_TRY(hipMemsetAsync(ctx->d_vars, 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
    for (uint32_t c = 0; c < ctx->n_cuts; c += 1)
    {
        HIP_TRY(hipMemsetAsync(ctx->cuts.pixels[c], 0, (size_t)ctx->n_pix * (S + 1) * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->cuts.avgs[c], 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->cuts.vars[c], 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
    }
    if (ctx->n_sensor)
    {
        const size_t n = ctx->n_sensor;
        HIP_TRY(hipMemsetAsync(ctx->sensor.pixels, 0, (size_t)ctx->n_pix * (n + 1) * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->sensor.avgs, 0, (size_t)ctx->n_pix * n * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->sensor.vars, 0, (size_t)ctx->n_pix * n * 8, ctx->stream));
    }
    for (uint32_t b = 0; b < ctx->n_buckets; b += 1)
    {
        HIP_TRY(hipMemsetAsync(ctx->buckets.pixels[b], 0, (size_t)ctx->n_pix * (S + 1) * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->buckets.avgs[b], 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->buckets.vars[b], 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
    }
    ctx->bk_samples = 0;
    for (uint32_t c = 0; c < ctx->n_lobes; c += 1)
    {
        HIP_TRY(hipMemsetAsync(ctx->lobes.pixels[c], 0, (size_t)ctx->n_pix * (S + 1) * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->lobes.avgs[c], 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->lobes.vars[c], 0, (size_t)ctx->n_pix * S * 8, ctx->stream));
    }
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, DRT_COUNTER_WORDS * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->film_used = ctx->adaptive_done = false;
    ctx->film_gen += 1;
    ctx->trace_ms = ctx->shade_ms = 0.0;
    ctx->timed_pairs = 0;
    ctx->min_sample_ms = ctx->max_sample_ms = ctx->avg_sample_ms = 0.0;
    return 0;
}

extern "C" int drt_film_device_ptrs(drt_context *ctx, void **d_pixels, void **d_avgs, void **d_vars)
{
    if (!ctx) return fail(-1, "null context");
    if (d_pixels) *d_pixels = ctx->d_pixels;
    if (d_avgs) *d_avgs = ctx->d_avgs;
    if (d_vars) *d_vars = ctx->d_vars;
    return 0;
}

extern "C" int drt_read_film(drt_context *ctx, double *pixels, double *avgs, double *vars)
{
    if (!ctx) return fail(-1, "null context");
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    const size_t S = ctx->dsc.S;
    if (ctx->xyz_mode && (avgs || vars)) return fail(-4, "the XYZ film has no mean / variance buffers");
    if (pixels) HIP_TRY(hipMemcpy(pixels, ctx->d_pixels, pixels_bytes(ctx), hipMemcpyDeviceToHost));
    if (avgs) HIP_TRY(hipMemcpy(avgs, ctx->d_avgs, (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    if (vars) HIP_TRY(hipMemcpy(vars, ctx->d_vars, (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_write_film(drt_context *ctx, const double *pixels, const double *avgs, const double *vars)
{
    if (!ctx) return fail(-1, "null context");
    if (ctx->adaptive_done) return fail(-7, "the film holds an adaptive render: drt_reset_film first");
    ctx->film_used = true;
    ctx->film_gen += 1;
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    const size_t S = ctx->dsc.S;
    if (ctx->xyz_mode && (avgs || vars)) return fail(-4, "the XYZ film has no mean / variance buffers");
    if (pixels) HIP_TRY(hipMemcpy(ctx->d_pixels, pixels, pixels_bytes(ctx), hipMemcpyHostToDevice));
    if (avgs) HIP_TRY(hipMemcpy(ctx->d_avgs, avgs, (size_t)ctx->n_pix * S * 8, hipMemcpyHostToDevice));
    if (vars) HIP_TRY(hipMemcpy(ctx->d_vars, vars, (size_t)ctx->n_pix * S * 8, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int drt_read_xyz(drt_context *ctx, double *xyz)
{
    if (!ctx || !xyz) return fail(-1, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    /* first the film itself: drt_synchronize is where a record pool that ran out is noticed and those samples are rendered again --
     * a conversion enqueued before it would read the incomplete film */
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    HIP_TRY(ctx->d_xyz.need((size_t)ctx->n_pix * 3));
    uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    if (ctx->xyz_mode)
        hipLaunchKernelGGL(drt_xyz_finish_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_y, ctx->interval,
                           ctx->n_pix, ctx->d_pixels, ctx->d_xyz);
    else
        hipLaunchKernelGGL(drt_film_xyz_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y,
                           ctx->cmf_z, ctx->interval, ctx->n_pix, ctx->d_pixels, ctx->d_xyz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(xyz, ctx->d_xyz, (size_t)ctx->n_pix * 3 * 8, hipMemcpyDeviceToHost));
    return 0;
}

/* one film buffer as BMP pixel bytes, left on the device in ctx->d_bgra */
static int film_to_bgra(drt_context *ctx, int which)
{
    if (which < 0 || which > 2) return fail(-1, "which = %d: 0 sum, 1 mean, 2 variance", which);
    if (ctx->xyz_mode) return fail(-4, "the XYZ film keeps no spectra: render in DRT_MODE_SPECTRAL for .bmp pixels");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = drt_synchronize(ctx); /* the complete film first (see drt_read_xyz) */
    if (rc) return rc;
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    const double *film = which == 0 ? ctx->d_pixels : which == 1 ? ctx->d_avgs : ctx->d_vars;
    uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_film_bgra_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y,
                       ctx->cmf_z, ctx->interval, ctx->n_pix, film, which, ctx->d_bgra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int drt_read_bgra(drt_context *ctx, int which, uint8_t *bgra)
{
    if (!ctx || !bgra) return fail(-1, "null argument");
    int rc = film_to_bgra(ctx, which);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_hit_indices(drt_context *ctx, int32_t *dst, uint64_t capacity_paths)
{
    if (!ctx || !dst) return fail(-1, "null argument");
    if (!(ctx->params.flags & DRT_FLAG_RECORD_HITS) || !ctx->d_hits) return fail(-4, "hit recording is off (DRT_FLAG_RECORD_HITS)");
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    uint64_t n = std::min<uint64_t>(capacity_paths, ctx->n_pix * (uint64_t)ctx->hits_samples);
    HIP_TRY(hipMemcpy(dst, ctx->d_hits, n * ctx->params.max_depth * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_get_stats(drt_context *ctx, drt_stats *out)
{
    if (!ctx || !out) return fail(-1, "null argument");
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    unsigned long long c[DRT_NUM_COUNTERS];
    HIP_TRY(hipMemcpy(c, ctx->d_counters, sizeof(c), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    out->paths = c[0];
    out->closest_hit_scans = c[1];
    out->shaded_vertices = c[2];
    out->shadow_scans = c[3];
    out->rng_draws = c[4];
    out->trace_ms = ctx->trace_ms;
    out->shade_ms = ctx->shade_ms;
    out->total_ms = ctx->trace_ms + ctx->shade_ms;
    out->record_pool_blocks = ctx->pool_blocks;
    out->record_pool_peak = ctx->pool_peak;
    out->record_block_bytes = ctx->block_words * 8;
    out->redone_launches = (uint32_t)ctx->redone_batches;
    out->launches = (uint32_t)std::min<uint64_t>(ctx->timed_pairs, 0xFFFFFFFFull);
    out->path_flags = (ctx->bvh_pipeline ? DRT_PATH_BVH : 0u) | ((ctx->trace_tail && ctx->d_tail_stage) ? DRT_PATH_TRACE_TAIL : 0u) |
                      (ctx->rays_bound ? DRT_PATH_RAYS : 0u) | ((ctx->trace_stash && !ctx->bvh_pipeline) ? DRT_PATH_RAY_STASH : 0u); /* the context's camera launches; DRT_PATH_RAYS says when those do not run */
    out->min_sample_ms = ctx->min_sample_ms;
    out->max_sample_ms = ctx->max_sample_ms;
    out->avg_sample_ms = ctx->avg_sample_ms;
    return 0;
}

extern "C" uint32_t drt_batch_spp(drt_context *ctx) { return ctx ? ctx->batch_spp : 0; }

static void window_out(const LiveWindow &w, uint32_t out[4]) { out[0] = w.x_lo; out[1] = w.x_hi; out[2] = w.y_lo; out[3] = w.y_hi; }

/* host only, like drt_bvh_stats: no device is touched */
extern "C" int drt_live_window_of(const drt_scene *scene, const drt_camera *camera, const drt_params *params, uint32_t out[4])
{
    g_last_error.clear();
    if (!scene || !camera || !params || !out) return fail(-1, "drt_live_window_of: null argument");
    if (scene->escape_material >= scene->num_materials) return fail(-2, "base/escape material index out of range");
    if ((uint64_t)params->x0 + params->tile_w > params->width ||
        (params->tile_h && (uint64_t)params->y0 + (uint64_t)(params->tile_h - 1) * (params->row_stride ? params->row_stride : 1) >= params->height))
        return fail(-1, "tile does not fit the %ux%u image", params->width, params->height);
    drt_params p = *params;
    if (p.row_stride == 0) p.row_stride = 1;
    window_out(live_window_of(scene->surfaces, scene->num_surfaces, scene->materials[scene->escape_material], *camera, p), out);
    return 0;
}

extern "C" int drt_live_window(drt_context *ctx, uint32_t out[4])
{
    if (!ctx || !out) return fail(-1, "drt_live_window: null argument");
    window_refresh(ctx);
    window_out(ctx->win, out);
    return 0;
}

extern "C" int drt_shade_instantiation(const drt_context *ctx)
{
    if (!ctx) return -1;
    if (shade_closed(ctx)) return DRT_SHADE_CLOSED;
    return shade_simple(ctx) ? DRT_SHADE_SIMPLE : DRT_SHADE_GENERAL;
}

extern "C" int drt_shade_closed_lds(const drt_context *ctx)
{
    if (!ctx) return -1;
    return shade_closed_lds(ctx) ? 1 : 0;
}

extern "C" int drt_shade_closed_waves(const drt_context *ctx)
{
    if (!ctx) return -1;
    if (!shade_closed(ctx)) return 0;
    return shade_closed_lds6(ctx) ? DRT_SHADE_WAVES_CLOSED_LDS6 : shade_closed_lds(ctx) ? DRT_SHADE_WAVES_CLOSED_LDS : DRT_SHADE_WAVES_CLOSED;
}

/*
 * Adaptive sampling ("Adaptive sampling"). Round 0 renders samples [0, min_spp) of every tile pixel through the dense
 * path; each later round renders the next min(step, max_spp - n) samples of the pixels still active, in kernel pairs over ranges of
 * the active list (the LIST instantiations), every pixel from the count it holds (d_counts). Every round ends with drt_converge_kernel
 * (+ scan + scatter), which takes the counts from the film's filter sums and writes the next list, and one read of two words: the
 * active count and the pixels at max_spp so far. A pixel rendered over samples 0 .. n-1 in order holds, bit for bit,
 * the film a uniform n-sample render gives it.
 */
static int adaptive_check(drt_context *ctx, const drt_adaptive *a, bool held = false) /* held: drt_render_adaptive_continue, on the film as it is */
{
    if (!ctx || !a) return fail(-1, "null argument");
    if (ctx->n_cuts) return fail(-4, "adaptive sampling with depth cuts bound is not supported: drt_bind_depth_cuts(ctx, NULL, 0) first");
    if (ctx->n_sensor) return fail(-4, "adaptive sampling with a sensor bound is not supported: drt_bind_sensor(ctx, NULL, 0) first");
    if (ctx->n_buckets) return fail(-4, "adaptive sampling with buckets bound is not supported: drt_bind_buckets(ctx, 0) first");
    if (ctx->n_lobes) return fail(-4, "adaptive sampling with lobes bound is not supported: drt_bind_lobes(ctx, 0, NULL) first");
    if (ctx->xyz_mode) return fail(-4, "adaptive sampling needs the spectral film (DRT_MODE_XYZ keeps no variance)");
    if (ctx->params.flags & DRT_FLAG_RECORD_HITS) return fail(-4, "adaptive sampling does not record hit indices (DRT_FLAG_RECORD_HITS)");
    if (!held && ctx->adaptive_done) return fail(-7, "the film holds an adaptive render: drt_reset_film first");
    if (!held && ctx->film_used) return fail(-7, "adaptive sampling needs a film without samples: drt_reset_film first");
    if (held && !ctx->adaptive_done && !ctx->film_used) return fail(-7, "the film holds no samples to continue from: drt_render_adaptive renders from the start");
    if (a->min_spp < 2) return fail(-1, "min_spp %u: at least 2 (the variance needs two samples)", a->min_spp);
    if (a->max_spp < a->min_spp) return fail(-1, "max_spp %u is below min_spp %u", a->max_spp, a->min_spp);
    if (a->step < 1) return fail(-1, "step must be at least 1");
    if (a->flags != 0) return fail(-1, "flags %u: none are defined", a->flags);
    if (!std::isfinite(a->rel_error) || !(a->rel_error > 0.0)) return fail(-1, "rel_error %g: a finite number above 0", a->rel_error);
    if (!std::isfinite(a->floor) || !(a->floor >= 0.0)) return fail(-1, "floor %g: a finite number, 0 or more", a->floor);
    if (ctx->n_pix > 0xFFFFFFFFull) return fail(-1, "adaptive sampling lists pixels in 32 bits: the tile has %llu", (unsigned long long)ctx->n_pix);
    return 0;
}

/* the convergence kernels over the round's n_in entries; the active count goes to d_bkeep[n_blocks] and from there, asynchronously, to
 * the pinned word h_active (adaptive_finish_round reads it after its wait) */
static int enqueue_converge(drt_context *ctx)
{
    drt_context::Adaptive &ad = ctx->ad;
    const uint32_t n_blocks = (uint32_t)(((uint64_t)ad.n_in + CONVERGE_BLOCK - 1) / CONVERGE_BLOCK);
    ConvergeParams cp{};
    cp.list_in = ad.first ? nullptr : ctx->d_alist[ad.cur];
    cp.n_in = ad.n_in;
    cp.max_spp = ad.a.max_spp;
    cp.cmf_rw = ctx->cmf_rw;
    cp.cmf_y = ctx->cmf_y;
    cp.interval = ctx->interval;
    cp.rel_error = ad.a.rel_error;
    cp.floor = ad.a.floor;
    cp.counts = ctx->d_counts;
    cp.keep_mask = ctx->d_keep;
    cp.block_keep = ctx->d_bkeep;
    cp.active = ctx->d_bkeep + n_blocks;
    cp.list_out = ctx->d_alist[ad.cur ^ 1];
    cp.overflow = (const uint32_t *)(ctx->d_counters + DRT_NUM_COUNTERS + 5);
    cp.pixels = ctx->d_pixels;
    cp.at_max = ctx->d_ainfo;
    hipLaunchKernelGGL(drt_converge_kernel, dim3(n_blocks), dim3(CONVERGE_BLOCK), 0, ctx->stream, ctx->dsc, cp, ctx->d_avgs, ctx->d_vars);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(drt_converge_scan, dim3(1), dim3(CONVERGE_SCAN_BLOCK), 0, ctx->stream, cp, n_blocks);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(drt_converge_scatter, dim3(n_blocks), dim3(CONVERGE_BLOCK), 0, ctx->stream, cp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_active, cp.active, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_active + 1, ctx->d_ainfo, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

static int adaptive_alloc(drt_context *ctx)
{
    const uint64_t n_pix = ctx->n_pix;
    HIP_TRY(ctx->d_counts.need(n_pix));
    HIP_TRY(ctx->d_alist[0].need(n_pix));
    HIP_TRY(ctx->d_alist[1].need(n_pix));
    HIP_TRY(ctx->d_keep.need((n_pix + 63) / 64));
    HIP_TRY(ctx->d_bkeep.need((n_pix + CONVERGE_BLOCK - 1) / CONVERGE_BLOCK + 1));
    HIP_TRY(ctx->d_ainfo.need(1 + ADOPT_WORDS));
    HIP_TRY(ctx->h_active.need(2 + ADOPT_WORDS));
    return 0;
}

/* the buffers of an adaptive render; the count of pixels at max_spp starts from zero */
static int adaptive_buffers(drt_context *ctx)
{
    if (!ctx->h_active) /* the last of the set, which is whole or absent */
    {
        /* all or none: a call that failed half way leaves no buffer behind that a later call would take for the whole set */
        const int rc = adaptive_alloc(ctx);
        if (rc)
        {
            for (DevBuf<uint32_t> *b : {&ctx->d_counts, &ctx->d_alist[0], &ctx->d_alist[1], &ctx->d_bkeep, &ctx->d_ainfo}) b->reset();
            ctx->d_keep.reset();
            return rc;
        }
    }
    HIP_TRY(hipMemsetAsync(ctx->d_ainfo, 0, sizeof(uint32_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_ainfo + 1 + ADOPT_BAD, 0xFF, sizeof(uint32_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_ainfo + 1 + ADOPT_MIN, 0xFF, sizeof(uint32_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_ainfo + 1 + ADOPT_MAX, 0, 2 * sizeof(uint32_t), ctx->stream));
    return 0;
}

/* round 0: buffers, the dense render of samples [0, min_spp), the convergence kernels */
static int adaptive_begin(drt_context *ctx, const drt_adaptive *a)
{
    HIP_TRY(hipSetDevice(ctx->device));
    (void)hipGetLastError();
    ctx->adaptive_done = true; /* from here on the film holds (part of) an adaptive render */
    drt_context::Adaptive &ad = ctx->ad;
    ad = drt_context::Adaptive{};
    ad.a = *a;
    ad.a.rounds = ad.a.pixels_at_max = 0;
    ad.a.paths = 0;
    const uint64_t n_pix = ctx->n_pix;
    int rc = adaptive_buffers(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ctx->d_counts, 0, n_pix * sizeof(uint32_t), ctx->stream));
    ad.first = true;
    ad.cur = 1; /* the first list goes to d_alist[0] */
    ad.n_in = (uint32_t)n_pix;
    ad.k = a->min_spp;
    ad.n = a->min_spp;
    if ((rc = render_impl(ctx, 0, a->min_spp))) return rc;
    return enqueue_converge(ctx);
}

/* a later round: the next k samples of the ad.active pixels of list d_alist[cur] -- each from the count it holds, d_counts -- in kernel
 * pairs over ranges of the list. k: min(step, max_spp - n) while all active pixels hold n samples, step otherwise (the contract). A pair
 * takes up to five eighths of the paths the record pool is sized for (the pixels still active are the ones with the long paths: a
 * pair that runs out anyway is rendered again by redo_batches), its pixels all the round's samples where they fit; pairs of equal size */
static int adaptive_enqueue_round(drt_context *ctx)
{
    drt_context::Adaptive &ad = ctx->ad;
    ad.first = false;
    ad.n_in = ad.active;
    ad.k = ad.same ? std::min(ad.a.step, ad.a.max_spp - ad.n) : ad.a.step;
    if (ad.same) ad.n += ad.k;
    const RoundPairs rp = round_pairs(ctx->n_pix, ctx->batch_spp, ad.k, ad.n_in);
    const uint32_t m = rp.m;
    const uint64_t P = rp.P;
    const uint32_t *list = ctx->d_alist[ad.cur];
    for (uint64_t off = 0; off < ad.n_in; off += P)
    {
        const uint64_t len = std::min<uint64_t>(P, ad.n_in - off);
        for (uint32_t at = 0; at < ad.k; at += m)
        {
            const uint32_t ns = std::min(m, ad.k - at);
            int rc = enqueue_pair(ctx, PairSpan::list_range(at, ns, list + off, len));
            if (rc) return rc;
        }
    }
    return enqueue_converge(ctx);
}

/* the round's one wait; a round whose record pool ran out is rendered again (drt_synchronize) and its convergence kernels rerun */
static int adaptive_finish_round(drt_context *ctx)
{
    drt_context::Adaptive &ad = ctx->ad;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint64_t redone = ctx->redone_batches;
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    if (ctx->redone_batches != redone)
    {
        if ((rc = enqueue_converge(ctx))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    ad.active = *ctx->h_active;
    ad.a.rounds += 1;
    ad.a.paths += (uint64_t)ad.n_in * (ad.first ? ad.a.min_spp : ad.k);
    ad.a.pixels_at_max = ctx->h_active[1];
    ad.cur ^= 1;
    return 0;
}

/* test knob DRT_ADAPTIVE_ROUNDS=k: stop after k rounds, the pixels still active left in the list drt_read_active_list reads */
static uint32_t adaptive_round_cap()
{
    const char *e = getenv("DRT_ADAPTIVE_ROUNDS");
    return e ? (uint32_t)std::max(0, atoi(e)) : 0u;
}

static bool adaptive_goes_on(const drt_context *ctx, uint32_t cap)
{
    return ctx->ad.active > 0 && !(cap && ctx->ad.a.rounds >= cap);
}

extern "C" int drt_render_adaptive(drt_context *ctx, drt_adaptive *a)
{
    g_last_error.clear();
    int rc = adaptive_check(ctx, a);
    if (rc) return rc;
    const uint32_t cap = adaptive_round_cap();
    if ((rc = adaptive_begin(ctx, a))) return rc;
    if ((rc = adaptive_finish_round(ctx))) return rc;
    while (adaptive_goes_on(ctx, cap))
    {
        if ((rc = adaptive_enqueue_round(ctx))) return rc;
        if ((rc = adaptive_finish_round(ctx))) return rc;
    }
    a->rounds = ctx->ad.a.rounds;
    a->pixels_at_max = ctx->ad.a.pixels_at_max;
    a->paths = ctx->ad.a.paths;
    return 0;
}

/*
 * drt_render_adaptive_continue: adaptive sampling on the film the context holds. In three steps, so that a group takes each of them on
 * all its devices before the next: continue_adopt (every tile pixel's count from its filter sum, checked), continue_test (every pixel
 * tested on its own rows, the first active list, the contract's three words over it), continue_accept (the context becomes an adaptive
 * render's; the rounds follow as in drt_render_adaptive). Until continue_accept nothing is rendered and no film bit changes, and a
 * refusal puts the context's earlier list back (continue_refuse).
 */
struct ContinueReport { uint32_t active = 0, lo = 0xFFFFFFFFu, hi = 0, rem = 0; };

static int continue_adopt(drt_context *ctx)
{
    HIP_TRY(hipSetDevice(ctx->device));
    (void)hipGetLastError();
    int rc = drt_synchronize(ctx); /* the film complete: samples of an earlier drt_render that ran out of records are rendered again here */
    if (rc) return rc;
    if ((rc = adaptive_buffers(ctx))) return rc;
    const uint32_t n_blocks = (uint32_t)((ctx->n_pix + CONVERGE_BLOCK - 1) / CONVERGE_BLOCK);
    hipLaunchKernelGGL(drt_adopt_counts_kernel, dim3(n_blocks), dim3(CONVERGE_BLOCK), 0, ctx->stream, ctx->d_pixels, ctx->dsc.S,
                       (uint32_t)ctx->n_pix, ctx->d_counts, ctx->d_ainfo + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_active + 2, ctx->d_ainfo + 1, ADOPT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

static int continue_test(drt_context *ctx, const drt_adaptive *a)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t bad = ctx->h_active[2 + ADOPT_BAD];
    if (bad != 0xFFFFFFFFu)
    {
        double f = 0.0;
        HIP_TRY(hipMemcpy(&f, ctx->d_pixels + (size_t)bad * (ctx->dsc.S + 1) + ctx->dsc.S, sizeof(f), hipMemcpyDeviceToHost));
        return fail(-7, "tile pixel %u (column %u, row %u of the tile) holds the filter sum %g: a sample count is a whole number from 2 to 2^32 - 1",
                    bad, bad % ctx->params.tile_w, bad / ctx->params.tile_w, f);
    }
    drt_context::Adaptive &ad = ctx->ad;
    const int cur = ctx->adaptive_done ? ad.cur : 1; /* the list an earlier call left stays where it is until this call is accepted */
    ad.a = *a;
    ad.a.rounds = ad.a.pixels_at_max = 0;
    ad.a.paths = 0;
    ad.cur = cur;
    ad.first = true;
    ad.n_in = (uint32_t)ctx->n_pix;
    int rc = enqueue_converge(ctx);
    if (rc) return rc;
    const uint32_t n_blocks = (uint32_t)((ctx->n_pix + CONVERGE_BLOCK - 1) / CONVERGE_BLOCK);
    hipLaunchKernelGGL(drt_contract_kernel, dim3(n_blocks), dim3(CONVERGE_BLOCK), 0, ctx->stream, ctx->d_alist[cur ^ 1], ctx->d_bkeep + n_blocks,
                       ctx->d_counts, a->max_spp, a->step, ctx->d_ainfo + 1, (const uint32_t *)(ctx->d_counters + DRT_NUM_COUNTERS + 5));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_active + 2, ctx->d_ainfo + 1, ADOPT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

static int continue_report(drt_context *ctx, ContinueReport *r)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    r->active += ctx->h_active[0];
    r->lo = std::min(r->lo, ctx->h_active[2 + ADOPT_MIN]);
    r->hi = std::max(r->hi, ctx->h_active[2 + ADOPT_MAX]);
    r->rem |= ctx->h_active[2 + ADOPT_REM];
    return 0;
}

/* the refusal's hint -- not on the way of a render, so on the host: the greatest common divisor of the active pixels' max_spp - count */
static int continue_gcd(drt_context *ctx, uint32_t max_spp, uint32_t *g)
{
    const uint32_t n = ctx->h_active[0];
    if (!n) return 0;
    std::vector<uint32_t> counts(ctx->n_pix), list(n);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(counts.data(), ctx->d_counts, ctx->n_pix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(list.data(), ctx->d_alist[ctx->ad.cur ^ 1], (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t t : list)
    {
        uint32_t x = max_spp - counts[t], y = *g;
        while (y) { const uint32_t r = x % y; x = y; y = r; }
        *g = x;
    }
    return 0;
}

static int continue_refuse(const ContinueReport &r, const drt_adaptive *a, uint32_t g)
{
    std::string steps;
    for (uint32_t d = 1; d <= g && steps.size() < 60; d += 1)
        if (g % d == 0) steps += (steps.empty() ? "" : ", ") + std::to_string(d);
    if (g > 1 && steps.size() >= 60) steps += ", ... (the divisors of " + std::to_string(g) + ")";
    return fail(-7, "the %u active pixels hold from %u to %u samples and max_spp %u less the count is not a multiple of step %u for all of them: "
                "a round renders the same number of samples of every active pixel, so step must be one of %s",
                r.active, r.lo, r.hi, a->max_spp, a->step, steps.c_str());
}

static void continue_accept(drt_context *ctx, const ContinueReport &r)
{
    drt_context::Adaptive &ad = ctx->ad;
    ctx->adaptive_done = true;
    ad.active = ctx->h_active[0];
    ad.a.pixels_at_max = ctx->h_active[1];
    ad.cur ^= 1;
    ad.first = false;
    ad.same = r.lo == r.hi;
    ad.n = r.lo;
    ad.k = 0;
}

static bool continue_goes_on(const drt_context *ctx, uint32_t max_rounds)
{
    return ctx->ad.active > 0 && !(max_rounds && ctx->ad.a.rounds >= max_rounds);
}

extern "C" int drt_render_adaptive_continue(drt_context *ctx, drt_adaptive *a, uint32_t max_rounds, uint32_t *still_active)
{
    g_last_error.clear();
    int rc = adaptive_check(ctx, a, true);
    if (rc) return rc;
    const drt_context::Adaptive before = ctx->ad;
    ContinueReport r;
    if ((rc = continue_adopt(ctx)) || (rc = continue_test(ctx, a)) || (rc = continue_report(ctx, &r)))
    {
        ctx->ad = before;
        return rc;
    }
    if (r.active && r.lo != r.hi && r.rem)
    {
        uint32_t g = 0;
        rc = continue_gcd(ctx, a->max_spp, &g);
        ctx->ad = before;
        return rc ? rc : continue_refuse(r, a, g);
    }
    continue_accept(ctx, r);
    while (continue_goes_on(ctx, max_rounds))
    {
        if ((rc = adaptive_enqueue_round(ctx))) return rc;
        if ((rc = adaptive_finish_round(ctx))) return rc;
    }
    a->rounds = ctx->ad.a.rounds;
    a->pixels_at_max = ctx->ad.a.pixels_at_max;
    a->paths = ctx->ad.a.paths;
    if (still_active) *still_active = ctx->ad.active;
    return 0;
}

extern "C" int drt_read_active_list(drt_context *ctx, uint32_t *list, uint32_t capacity, uint32_t *count)
{
    if (!ctx || !count || (!list && capacity)) return fail(-1, "null argument");
    if (!ctx->adaptive_done || !ctx->d_counts) return fail(-4, "no adaptive render: the list comes from drt_render_adaptive");
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    const uint32_t n = ctx->ad.active;
    if (n > capacity) return fail(-1, "the active list holds %u entries, the buffer %u", n, capacity);
    if (n) HIP_TRY(hipMemcpy(list, ctx->d_alist[ctx->ad.cur], (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *count = n;
    return 0;
}

extern "C" int drt_read_sample_counts(drt_context *ctx, uint32_t *counts)
{
    if (!ctx || !counts) return fail(-1, "null argument");
    if (!ctx->adaptive_done || !ctx->d_counts) return fail(-4, "no adaptive render: the counts come from drt_render_adaptive");
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(counts, ctx->d_counts, ctx->n_pix * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

static double wall_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

extern "C" int drt_render_tile(const drt_scene *scene, const drt_camera *camera, const drt_params *params,
                               double *dst_pixels, double *dst_avgs, double *dst_vars, drt_stats *stats)
{
    g_last_error.clear();
    const bool xyz = params && params->mode == DRT_MODE_XYZ; /* then dst_pixels is [n][8] and the other two are not used */
    if (!dst_pixels || (!xyz && (!dst_avgs || !dst_vars))) return fail(-1, "null film buffer");
    if (xyz) dst_avgs = dst_vars = nullptr;
    const bool verbose = getenv("DRT_VERBOSE") != nullptr || getenv("DRT_TIMING") != nullptr;
    double t[6] = {wall_ms(), 0, 0, 0, 0, 0};
    drt_context *ctx = drt_create(scene, camera, params);
    if (!ctx) return -1;
    t[1] = wall_ms();
    int rc = 0;
    do
    {
        /* accumulate INTO the caller's buffers: start from their contents (unless the caller vouches they are zero) */
        if (!(params->flags & DRT_FLAG_FILM_ZERO) && (rc = drt_write_film(ctx, dst_pixels, dst_avgs, dst_vars))) break;
        t[2] = wall_ms();
        /* The tile goes out in row blocks, each with all its samples (as many per kernel pair as the record pool was sized for: a
         * quarter of the rows takes four times the samples), so that a block's film rows cross PCIe while the next block renders:
         * what is left exposed of the 1.7 GB download is its last quarter. (A pool that runs out on the way: drt_synchronize
         * renders again from there, and the film is fetched whole.) */
        uint32_t n_blocks = 8; /* 1024^2 x 256 spp, wall: 226 ms in one piece, 219 / 214 / 206 ms in 2 / 4 / 8 blocks (kernels 187 -> 197 ms: smaller launches) */
        if (getenv("DRT_ONESHOT_BLOCKS")) n_blocks = (uint32_t)std::max(1, atoi(getenv("DRT_ONESHOT_BLOCKS")));
        const uint32_t per = row_block_rows(ctx->params.tile_h, n_blocks); /* rows per block */
        const bool blocks_ok = params->spp != 0 && n_blocks > 1 && !(params->flags & DRT_FLAG_RECORD_HITS) && ctx->params.tile_h >= 16 * n_blocks &&
                               (uint64_t)ctx->params.tile_w * ctx->params.tile_h >= (1u << 18);
        std::vector<Event> block_done;
        if (!blocks_ok)
        {
            if ((rc = drt_render(ctx, params->first_sample, params->spp))) break;
        }
        else
        {
            if ((rc = window_open(ctx))) break;
            rc = enqueue_blocks(ctx, params->first_sample, params->spp, n_blocks, &block_done);
            window_close(ctx);
            if (rc) break;
        }
        if (params->flags & DRT_FLAG_FILM_ZERO)
        {
            /* Buffers that come zero-filled (the reference's alloc()) have usually never been touched: the download would then
             * pay a page fault per 4 KB (100 ms for 1.7 GB instead of 30). The kernels are running and this thread has nothing to
             * do, so it touches the pages now -- writing the zero the caller vouched for into one byte of each. */
            const size_t n = (size_t)params->tile_w * params->tile_h, S = scene->num_wavelengths;
            char *bufs[3] = {(char *)dst_pixels, (char *)dst_avgs, (char *)dst_vars};
            const size_t sizes[3] = {n * (xyz ? (size_t)XYZ_FILM_WORDS : S + 1) * 8, n * S * 8, n * S * 8};
            for (int k = 0; k < 3; k += 1)
            {
                if (!bufs[k]) continue;
                for (size_t off = 0; off < sizes[k]; off += 4096) ((volatile char *)bufs[k])[off] = 0;
                if (sizes[k]) ((volatile char *)bufs[k])[sizes[k] - 1] = 0;
            }
        }
        if (verbose && !blocks_ok && (rc = drt_synchronize(ctx))) break;
        t[3] = wall_ms();
        bool fetched = false;
        if (blocks_ok && block_done.size() == (size_t)((ctx->params.tile_h + per - 1) / per))
        {
            const size_t W = ctx->params.tile_w, S = scene->num_wavelengths;
            const size_t words[3] = {xyz ? (size_t)XYZ_FILM_WORDS : S + 1, S, S};
            double *host[3] = {dst_pixels, dst_avgs, dst_vars};
            double *dev[3] = {ctx->d_pixels, ctx->d_avgs, ctx->d_vars};
            fetched = true;
            for (size_t k = 0; k < block_done.size() && fetched; k += 1)
            {
                if (hipEventSynchronize(block_done[k]) != hipSuccess) { fetched = false; break; }
                unsigned long long st[4] = {0, 0, 0, 0}; /* pool cursor, overflow flag, last complete pair, peak */
                if (hipMemcpy(st, ctx->d_counters + DRT_NUM_COUNTERS + 4, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess || (uint32_t)st[1] != 0u) { fetched = false; break; }
                const size_t r0 = k * per, rows = std::min<size_t>(per, ctx->params.tile_h - r0);
                for (int f = 0; f < 3; f += 1)
                    if (host[f] && dev[f] && hipMemcpy(host[f] + r0 * W * words[f], dev[f] + r0 * W * words[f], rows * W * words[f] * 8, hipMemcpyDeviceToHost) != hipSuccess) fetched = false;
            }
        }
        block_done.clear();
        if ((rc = drt_synchronize(ctx))) break; /* timings, and what a pool that ran out left undone */
        if (!fetched && (rc = drt_read_film(ctx, dst_pixels, dst_avgs, dst_vars))) break;
        if (stats && (rc = drt_get_stats(ctx, stats))) break;
        t[4] = wall_ms();
    } while (0);
    std::string keep = g_last_error;
    drt_destroy(ctx);
    g_last_error = keep;
    t[5] = wall_ms();
    if (verbose && rc == 0)
        fprintf(stderr, "drt_render_tile: create %.1f ms, film upload %.1f ms, render %.1f ms, film download %.1f ms, destroy %.1f ms\n",
                t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4]);
    return rc;
}

/* ---------------------------------------------------------------------------------------------- */
/* Device groups: one host thread, several GPUs                                                     */

struct drt_group
{
    std::vector<drt_context *> ctx; /* nullptr for a device that got no rows */
    std::vector<uint32_t>      rows;
    uint32_t tile_w = 0, tile_h = 0, S = 0;
    bool     xyz_mode = false;
};

extern "C" void drt_group_destroy(drt_group *g)
{
    if (!g) return;
    std::string keep = g_last_error;
    for (drt_context *c : g->ctx) drt_destroy(c);
    delete g;
    g_last_error = keep;
}

extern "C" drt_group *drt_group_create(const drt_scene *scene, const drt_camera *camera, const drt_params *params,
                                       const int32_t *devices, uint32_t n_devices)
{
    g_last_error.clear();
    if (!scene || !camera || !params)
    {
        fail(-1, "null argument");
        return nullptr;
    }
    if (n_devices == 0)
    {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        {
            (void)hipGetLastError();
            fail(-5, "no HIP device is visible");
            return nullptr;
        }
        n_devices = (uint32_t)n;
        devices = nullptr;
    }
    if (n_devices > 64)
    {
        fail(-1, "more than 64 devices in a group");
        return nullptr;
    }
    if (params->flags & DRT_FLAG_RECORD_HITS)
    {
        fail(-1, "hit recording is per context: use drt_create for it");
        return nullptr;
    }
    drt_group *g = new drt_group();
    g->tile_w = params->tile_w;
    g->tile_h = params->tile_h;
    g->S = scene->num_wavelengths;
    g->xyz_mode = params->mode == DRT_MODE_XYZ;
    for (uint32_t k = 0; k < n_devices; k += 1)
    {
        drt_params p = *params;
        p.device = devices ? devices[k] : (int32_t)k;
        p.y0 = params->y0 + k * params->row_stride;
        p.row_stride = params->row_stride * n_devices;
        p.tile_h = params->tile_h > k ? (params->tile_h - k + n_devices - 1) / n_devices : 0;
        g->rows.push_back(p.tile_h);
        if (p.tile_h == 0)
        {
            g->ctx.push_back(nullptr);
            continue;
        }
        drt_context *c = drt_create(scene, camera, &p);
        if (!c)
        {
            drt_group_destroy(g);
            return nullptr;
        }
        g->ctx.push_back(c);
    }
    return g;
}

extern "C" uint32_t drt_group_size(drt_group *g) { return g ? (uint32_t)g->ctx.size() : 0; }

extern "C" int drt_group_render(drt_group *g, uint32_t first_sample, uint32_t num_samples)
{
    if (!g) return fail(-1, "null group");
    for (drt_context *c : g->ctx)
        if (c)
        {
            int rc = drt_render(c, first_sample, num_samples); /* asynchronous: the devices run side by side */
            if (rc) return rc;
        }
    return 0;
}

extern "C" int drt_group_synchronize(drt_group *g)
{
    if (!g) return fail(-1, "null group");
    for (drt_context *c : g->ctx)
        if (c)
        {
            int rc = drt_synchronize(c);
            if (rc) return rc;
        }
    return 0;
}

extern "C" int drt_group_reset_film(drt_group *g)
{
    if (!g) return fail(-1, "null group");
    for (drt_context *c : g->ctx)
        if (c)
        {
            int rc = drt_reset_film(c);
            if (rc) return rc;
        }
    return 0;
}

/* Of n devices, device k holds rows k, k + n, ... of the tile, contiguously in the buffer `buf` of its context: rows of row_bytes
 * bytes of a whole-tile host buffer <-> every device's own, one strided copy per device. A null host buffer is left out.
 * B: a DevBuf<T>, or the double * of a film member. */
template <typename B>
static int group_move_rows(drt_group *g, void *host, size_t row_bytes, B drt_context::*buf, bool to_device)
{
    if (!host) return 0;
    const size_t n = g->ctx.size();
    for (size_t k = 0; k < n; k += 1)
    {
        drt_context *c = g->ctx[k];
        if (!c) continue;
        HIP_TRY(hipSetDevice(c->device));
        char *h = (char *)host + k * row_bytes;
        void *dev = c->*buf;
        if (to_device)
            HIP_TRY(hipMemcpy2D(dev, row_bytes, h, n * row_bytes, row_bytes, g->rows[k], hipMemcpyHostToDevice));
        else
            HIP_TRY(hipMemcpy2D(h, n * row_bytes, dev, row_bytes, row_bytes, g->rows[k], hipMemcpyDeviceToHost));
    }
    return 0;
}
template <typename B>
static int group_gather_rows(drt_group *g, void *host, size_t row_bytes, B drt_context::*buf) { return group_move_rows(g, host, row_bytes, buf, false); }
template <typename B>
static int group_scatter_rows(drt_group *g, const void *host, size_t row_bytes, B drt_context::*buf)
{
    return group_move_rows(g, const_cast<void *>(host), row_bytes, buf, true);
}

/* which: 0 the film's sums, 1 the running means, 2 the variances */
static int group_copy(drt_group *g, double *host, int which, bool to_device)
{
    if (!host) return 0;
    const size_t C = which == 0 ? (g->xyz_mode ? (size_t)XYZ_FILM_WORDS : (size_t)g->S + 1) : (size_t)g->S;
    if (g->xyz_mode && which != 0) return fail(-4, "the XYZ film has no mean / variance buffers");
    double *drt_context::*buf = which == 0 ? &drt_context::d_pixels : which == 1 ? &drt_context::d_avgs : &drt_context::d_vars;
    const size_t row_bytes = (size_t)g->tile_w * C * 8;
    return to_device ? group_scatter_rows(g, host, row_bytes, buf) : group_gather_rows(g, host, row_bytes, buf);
}

extern "C" int drt_group_read_film(drt_group *g, double *pixels, double *avgs, double *vars)
{
    int rc = drt_group_synchronize(g);
    if (rc) return rc;
    if ((rc = group_copy(g, pixels, 0, false))) return rc;
    if ((rc = group_copy(g, avgs, 1, false))) return rc;
    return group_copy(g, vars, 2, false);
}

extern "C" int drt_group_write_film(drt_group *g, const double *pixels, const double *avgs, const double *vars)
{
    int rc = drt_group_synchronize(g);
    if (rc) return rc;
    for (drt_context *c : g->ctx)
        if (c && c->adaptive_done) return fail(-7, "the film holds an adaptive render: drt_reset_film first");
    for (drt_context *c : g->ctx)
        if (c)
        {
            c->film_used = true;
            c->film_gen += 1;
        }
    if ((rc = group_copy(g, const_cast<double *>(pixels), 0, true))) return rc;
    if ((rc = group_copy(g, const_cast<double *>(avgs), 1, true))) return rc;
    return group_copy(g, const_cast<double *>(vars), 2, true);
}

extern "C" int drt_group_read_bgra(drt_group *g, int which, uint8_t *bgra)
{
    if (!g || !bgra) return fail(-1, "null argument");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = film_to_bgra(c, which))) return rc;
    return group_gather_rows(g, bgra, (size_t)g->tile_w * 4, &drt_context::d_bgra);
}

extern "C" int drt_group_get_stats(drt_group *g, drt_stats *out)
{
    if (!g || !out) return fail(-1, "null argument");
    memset(out, 0, sizeof(*out));
    for (drt_context *c : g->ctx)
    {
        if (!c) continue;
        drt_stats st;
        int rc = drt_get_stats(c, &st);
        if (rc) return rc;
        out->paths += st.paths;
        out->closest_hit_scans += st.closest_hit_scans;
        out->shaded_vertices += st.shaded_vertices;
        out->shadow_scans += st.shadow_scans;
        out->rng_draws += st.rng_draws;
        out->trace_ms = std::max(out->trace_ms, st.trace_ms);
        out->shade_ms = std::max(out->shade_ms, st.shade_ms);
        out->total_ms = std::max(out->total_ms, st.total_ms);
        out->record_pool_blocks += st.record_pool_blocks; /* all the pools together; the fullest any of them has been */
        out->record_pool_peak = std::max(out->record_pool_peak, st.record_pool_peak);
        out->record_block_bytes = st.record_block_bytes;
        out->redone_launches += st.redone_launches;
        /* the devices run side by side: a sample pass over the whole tile takes as long as the slowest device's share */
        out->launches += st.launches;
        out->path_flags |= st.path_flags;
        out->min_sample_ms = std::max(out->min_sample_ms, st.min_sample_ms);
        out->max_sample_ms = std::max(out->max_sample_ms, st.max_sample_ms);
        out->avg_sample_ms = std::max(out->avg_sample_ms, st.avg_sample_ms);
    }
    return 0;
}

/* every device its own rounds on its own rows, side by side: a round is enqueued on all of them before any is waited for */
extern "C" int drt_group_render_adaptive(drt_group *g, drt_adaptive *a)
{
    g_last_error.clear();
    if (!g || !a) return fail(-1, "null argument");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = adaptive_check(c, a))) return rc;
    const uint32_t cap = adaptive_round_cap();
    std::vector<char> running(g->ctx.size(), 0); /* a round of this device is in flight */
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k])
        {
            if ((rc = adaptive_begin(g->ctx[k], a))) return rc;
            running[k] = 1;
        }
    for (;;)
    {
        for (size_t k = 0; k < g->ctx.size(); k += 1)
            if (running[k] && (rc = adaptive_finish_round(g->ctx[k]))) return rc;
        bool any = false;
        for (size_t k = 0; k < g->ctx.size(); k += 1)
        {
            running[k] = g->ctx[k] && adaptive_goes_on(g->ctx[k], cap);
            if (running[k] && (rc = adaptive_enqueue_round(g->ctx[k]))) return rc;
            any = any || running[k];
        }
        if (!any) break;
    }
    a->rounds = 0;
    a->pixels_at_max = 0;
    a->paths = 0;
    for (drt_context *c : g->ctx)
        if (c)
        {
            a->rounds = std::max(a->rounds, c->ad.a.rounds);
            a->pixels_at_max += c->ad.a.pixels_at_max;
            a->paths += c->ad.a.paths;
        }
    return 0;
}

/* parameters checked, films adopted and the contract decided over the whole tile on all devices before any device renders */
extern "C" int drt_group_render_adaptive_continue(drt_group *g, drt_adaptive *a, uint32_t max_rounds, uint32_t *still_active)
{
    g_last_error.clear();
    if (!g || !a) return fail(-1, "null argument");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = adaptive_check(c, a, true))) return rc;
    std::vector<drt_context::Adaptive> before;
    for (drt_context *c : g->ctx) before.push_back(c ? c->ad : drt_context::Adaptive{});
    auto put_back = [&]() { for (size_t k = 0; k < g->ctx.size(); k += 1) if (g->ctx[k]) g->ctx[k]->ad = before[k]; };
    ContinueReport r;
    for (drt_context *c : g->ctx)
        if (c && (rc = continue_adopt(c))) { put_back(); return rc; }
    for (drt_context *c : g->ctx)
        if (c && (rc = continue_test(c, a))) { put_back(); return rc; }
    for (drt_context *c : g->ctx)
        if (c && (rc = continue_report(c, &r))) { put_back(); return rc; }
    if (r.active && r.lo != r.hi && r.rem)
    {
        uint32_t d = 0;
        for (drt_context *c : g->ctx)
            if (c && !rc) rc = continue_gcd(c, a->max_spp, &d);
        put_back();
        return rc ? rc : continue_refuse(r, a, d);
    }
    for (drt_context *c : g->ctx)
        if (c) continue_accept(c, r);
    std::vector<char> running(g->ctx.size(), 0);
    for (;;)
    {
        bool any = false;
        for (size_t k = 0; k < g->ctx.size(); k += 1)
        {
            running[k] = g->ctx[k] && continue_goes_on(g->ctx[k], max_rounds);
            if (running[k] && (rc = adaptive_enqueue_round(g->ctx[k]))) return rc;
            any = any || running[k];
        }
        if (!any) break;
        for (size_t k = 0; k < g->ctx.size(); k += 1)
            if (running[k] && (rc = adaptive_finish_round(g->ctx[k]))) return rc;
    }
    a->rounds = 0;
    a->pixels_at_max = 0;
    a->paths = 0;
    uint32_t left = 0;
    for (drt_context *c : g->ctx)
        if (c)
        {
            a->rounds = std::max(a->rounds, c->ad.a.rounds);
            a->pixels_at_max += c->ad.a.pixels_at_max;
            a->paths += c->ad.a.paths;
            left += c->ad.active;
        }
    if (still_active) *still_active = left;
    return 0;
}

extern "C" int drt_group_read_sample_counts(drt_group *g, uint32_t *counts)
{
    if (!g || !counts) return fail(-1, "null argument");
    for (drt_context *c : g->ctx)
    {
        if (!c) continue;
        if (!c->adaptive_done || !c->d_counts) return fail(-4, "no adaptive render: the counts come from drt_group_render_adaptive");
        int rc = drt_synchronize(c);
        if (rc) return rc;
    }
    return group_gather_rows(g, counts, (size_t)g->tile_w * sizeof(uint32_t), &drt_context::d_counts);
}

/* ---------------------------------------------------------------------------------------------- */
/* Sample maps (the kernels in drt_sample_map_kernels.h)                      */

/*
 * drt_render_sample_map in steps, so that a group takes each of them on all its devices before the next: map_check, map_adopt (the
 * film complete, counts and remainders of every tile pixel, the report on its way to the host), map_report (the report's words
 * combined; its two refusals), map_accept (the context becomes an adaptive render's and the first round's list is enqueued),
 * then per round map_enqueue_round and map_finish_round. Until map_accept nothing is rendered and no film bit changes.
 * A round is its kernel pairs over ranges of the list and, behind them, the NEXT round's select + scan + scatter (after the last round:
 * a select that keeps nothing, which leaves the counts current and the list empty): one host wait per round, and one before the first
 * for its list's length. The select does nothing when a pair ran out of records; the finish renders those pairs again and reruns it.
 */
struct MapReport { uint32_t bits = 0, max_count = 0, rendered = 0, above = 0; uint64_t paths = 0; };

static int map_check(const drt_context *ctx, const drt_sample_map *m, bool group)
{
    if (!ctx || !m || !m->targets) return fail(-1, "null argument");
    if (m->flags & ~(DRT_MAP_DEVICE | DRT_MAP_ADD)) return fail(-1, "flags %u: DRT_MAP_DEVICE and DRT_MAP_ADD are defined", m->flags);
    if (group && (m->flags & DRT_MAP_DEVICE)) return fail(-1, "a group takes the map from host memory (DRT_MAP_DEVICE is per context)");
    if (ctx->n_cuts) return fail(-4, "sample maps with depth cuts bound are not supported: drt_bind_depth_cuts(ctx, NULL, 0) first");
    if (ctx->n_sensor) return fail(-4, "sample maps with a sensor bound are not supported: drt_bind_sensor(ctx, NULL, 0) first");
    if (ctx->n_buckets) return fail(-4, "sample maps with buckets bound are not supported: drt_bind_buckets(ctx, 0) first");
    if (ctx->n_lobes) return fail(-4, "sample maps with lobes bound are not supported: drt_bind_lobes(ctx, 0, NULL) first");
    if (ctx->xyz_mode) return fail(-4, "sample maps need the spectral film (the DRT_MODE_XYZ film keeps no filter sum per pixel)");
    if (ctx->params.flags & DRT_FLAG_RECORD_HITS) return fail(-4, "sample maps do not record hit indices (DRT_FLAG_RECORD_HITS)");
    if (ctx->n_pix > 0xFFFFFFFFull) return fail(-1, "sample maps list pixels in 32 bits: the tile has %llu", (unsigned long long)ctx->n_pix);
    return 0;
}

/* what a call made is given up when the call is refused: a refusal leaves the process's live resources as they were */
struct MapMade { bool adaptive = false, map = false; };

static void map_drop(drt_context *ctx, const MapMade &made)
{
    if (made.adaptive)
    {
        for (DevBuf<uint32_t> *b : {&ctx->d_counts, &ctx->d_alist[0], &ctx->d_alist[1], &ctx->d_bkeep, &ctx->d_ainfo}) b->reset();
        ctx->d_keep.reset();
        ctx->h_active.reset();
    }
    if (made.map)
    {
        for (DevBuf<uint32_t> *b : {&ctx->d_sm_rem, &ctx->d_sm_targets, &ctx->d_sm_report}) b->reset();
        ctx->h_sm_report.reset();
    }
}

static int map_alloc(drt_context *ctx)
{
    HIP_TRY(ctx->d_sm_rem.need(ctx->n_pix));
    HIP_TRY(ctx->d_sm_targets.need(ctx->n_pix));
    HIP_TRY(ctx->d_sm_report.need(MAP_WORDS));
    HIP_TRY(ctx->h_sm_report.need(MAP_WORDS));
    return 0;
}

/* targets: device memory on the context's device (the caller's, or d_sm_targets filled by the caller of this function) */
static int map_adopt(drt_context *ctx, const uint32_t *host_targets, const uint32_t *dev_targets, uint32_t flags, MapMade *made)
{
    HIP_TRY(hipSetDevice(ctx->device));
    (void)hipGetLastError();
    int rc = drt_synchronize(ctx); /* the film complete: samples of an earlier call that ran out of records are rendered again here */
    if (rc) return rc;
    made->adaptive = !ctx->h_active;
    made->map = !ctx->h_sm_report; /* the last of the set, which is whole or absent */
    if ((rc = adaptive_buffers(ctx))) { made->adaptive = false; return rc; } /* (all or none already) */
    if (made->map && (rc = map_alloc(ctx)))
    {
        map_drop(ctx, *made);
        return rc;
    }
    HIP_TRY(hipMemsetAsync(ctx->d_sm_report, 0xFF, 2 * sizeof(uint32_t), ctx->stream)); /* MAP_BAD, MAP_OVER */
    HIP_TRY(hipMemsetAsync(ctx->d_sm_report + 2, 0, (MAP_WORDS - 2) * sizeof(uint32_t), ctx->stream));
    if (host_targets)
    {
        /* (the caller's memory stays as it is until map_report has waited for the stream) */
        HIP_TRY(hipMemcpyAsync(ctx->d_sm_targets, host_targets, ctx->n_pix * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        dev_targets = ctx->d_sm_targets;
    }
    const uint32_t n_blocks = (uint32_t)((ctx->n_pix + CONVERGE_BLOCK - 1) / CONVERGE_BLOCK);
    hipLaunchKernelGGL(drt_map_adopt_kernel, dim3(n_blocks), dim3(CONVERGE_BLOCK), 0, ctx->stream, (const double *)ctx->d_pixels, ctx->dsc.S,
                       (uint32_t)ctx->n_pix, dev_targets, (flags & DRT_MAP_ADD) ? 1u : 0u, ctx->d_counts.get(), ctx->d_sm_rem.get(),
                       ctx->d_sm_report.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_sm_report, ctx->d_sm_report, MAP_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

static int map_report(drt_context *ctx, MapReport *r)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t *w = ctx->h_sm_report;
    const uint32_t W = ctx->params.tile_w;
    if (w[MAP_BAD] != 0xFFFFFFFFu)
    {
        const uint32_t bad = w[MAP_BAD];
        double f = 0.0;
        HIP_TRY(hipMemcpy(&f, ctx->d_pixels + (size_t)bad * (ctx->dsc.S + 1) + ctx->dsc.S, sizeof(f), hipMemcpyDeviceToHost));
        return fail(-7, "tile pixel %u (column %u, row %u of the tile) holds the filter sum %g: a sample count is a whole number from 0 to 2^32 - 1",
                    bad, bad % W, bad / W, f);
    }
    if (w[MAP_OVER] != 0xFFFFFFFFu)
    {
        const uint32_t at = w[MAP_OVER];
        uint32_t n = 0;
        HIP_TRY(hipMemcpy(&n, ctx->d_counts + at, sizeof(n), hipMemcpyDeviceToHost));
        return fail(-1, "tile pixel %u (column %u, row %u of the tile) holds %u samples and DRT_MAP_ADD asks for more than the %u that take it to 2^32 - 1",
                    at, at % W, at / W, n, 0xFFFFFFFFu - n);
    }
    r->bits |= w[MAP_BITS];
    r->max_count = std::max(r->max_count, w[MAP_MAX]);
    r->rendered += w[MAP_RENDERED];
    r->above += w[MAP_ABOVE];
    r->paths += (uint64_t)w[MAP_PATHS] | ((uint64_t)w[MAP_PATHS + 1] << 32);
    return 0;
}

/* select + scan + scatter for round b over every tile pixel, the list to d_alist[cur ^ 1], its length on its way to h_active */
static int map_enqueue_select(drt_context *ctx, uint32_t b)
{
    drt_context::Adaptive &ad = ctx->ad;
    const uint32_t n_pix = (uint32_t)ctx->n_pix;
    const uint32_t n_blocks = (uint32_t)((ctx->n_pix + CONVERGE_BLOCK - 1) / CONVERGE_BLOCK);
    ConvergeParams cp{};
    cp.list_in = nullptr;
    cp.n_in = n_pix;
    cp.counts = ctx->d_counts;
    cp.keep_mask = ctx->d_keep;
    cp.block_keep = ctx->d_bkeep;
    cp.active = ctx->d_bkeep + n_blocks;
    cp.list_out = ctx->d_alist[ad.cur ^ 1];
    cp.overflow = (const uint32_t *)(ctx->d_counters + DRT_NUM_COUNTERS + 5);
    cp.pixels = ctx->d_pixels;
    hipLaunchKernelGGL(drt_map_select_kernel, dim3(n_blocks), dim3(CONVERGE_BLOCK), 0, ctx->stream, (const double *)ctx->d_pixels, ctx->dsc.S, n_pix,
                       (const uint32_t *)ctx->d_sm_rem, b, cp.counts, cp.keep_mask, cp.block_keep, cp.overflow);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(drt_converge_scan, dim3(1), dim3(CONVERGE_SCAN_BLOCK), 0, ctx->stream, cp, n_blocks);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(drt_converge_scatter, dim3(n_blocks), dim3(CONVERGE_BLOCK), 0, ctx->stream, cp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_active, cp.active, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

static uint32_t lowest_bit(uint32_t bits) { return bits ? (uint32_t)__builtin_ctz(bits) : 32u; }

/* the context becomes an adaptive render's, its counts the adopted ones; a device with rounds to run gets its first list enqueued */
static int map_accept(drt_context *ctx)
{
    drt_context::Adaptive &ad = ctx->ad;
    const int cur = ctx->adaptive_done ? ad.cur : 1;
    ctx->adaptive_done = true;
    ad = drt_context::Adaptive{};
    ad.cur = cur;
    ad.first = false;
    ctx->sm_bits = ctx->h_sm_report[MAP_BITS];
    if (!ctx->sm_bits) return 0; /* nothing to render: the list stays empty (ad.active == 0) */
    HIP_TRY(hipSetDevice(ctx->device));
    return map_enqueue_select(ctx, lowest_bit(ctx->sm_bits));
}

/* the list's length (the wait before the first round) */
static int map_first_list(drt_context *ctx)
{
    if (!ctx->sm_bits) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->ad.active = *ctx->h_active;
    ctx->ad.cur ^= 1;
    return 0;
}

/* the round of the lowest bit left: 2^b samples of the listed pixels, each from the count it holds, then the next round's list */
static int map_enqueue_round(drt_context *ctx)
{
    drt_context::Adaptive &ad = ctx->ad;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t b = lowest_bit(ctx->sm_bits);
    ctx->sm_bits &= ctx->sm_bits - 1u;
    ad.n_in = ad.active;
    ad.k = 1u << b;
    const RoundPairs rp = round_pairs(ctx->n_pix, ctx->batch_spp, ad.k, ad.n_in);
    const uint32_t *list = ctx->d_alist[ad.cur];
    for (uint64_t off = 0; off < ad.n_in; off += rp.P)
    {
        const uint64_t len = std::min<uint64_t>(rp.P, ad.n_in - off);
        for (uint32_t at = 0; at < ad.k; at += rp.m)
        {
            int rc = 0;
            /* the pending timing events stay bounded (a round of 2^31 samples is half a million pairs): the counts and the list are
             * the round's until its select runs, so pairs redone here start where they started */
            if (ctx->ev_used >= 3 * 256 && (rc = drt_synchronize(ctx))) return rc;
            const uint32_t ns = std::min(rp.m, ad.k - at);
            if ((rc = enqueue_pair(ctx, PairSpan::list_range(at, ns, list + off, len)))) return rc;
        }
    }
    return map_enqueue_select(ctx, lowest_bit(ctx->sm_bits));
}

/* the round's one wait; pairs whose record pool ran out are rendered again (drt_synchronize) and the select they held back rerun */
static int map_finish_round(drt_context *ctx)
{
    drt_context::Adaptive &ad = ctx->ad;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint64_t redone = ctx->redone_batches;
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    if (ctx->redone_batches != redone)
    {
        if ((rc = map_enqueue_select(ctx, lowest_bit(ctx->sm_bits)))) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    ad.active = *ctx->h_active;
    ad.cur ^= 1;
    return 0;
}

static void map_fill(drt_sample_map *m, const MapReport &r)
{
    m->rounds = (uint32_t)__builtin_popcount(r.bits);
    m->pixels_rendered = r.rendered;
    m->pixels_above = r.above;
    m->max_count = r.max_count;
    m->paths = r.paths;
}

extern "C" int drt_render_sample_map(drt_context *ctx, drt_sample_map *m)
{
    g_last_error.clear();
    int rc = map_check(ctx, m, false);
    if (rc) return rc;
    const bool device = (m->flags & DRT_MAP_DEVICE) != 0;
    if (device)
    {
        HIP_TRY(hipSetDevice(ctx->device));
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, m->targets) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->device)
        {
            (void)hipGetLastError();
            return fail(-1, "DRT_MAP_DEVICE: targets is not device memory on the context's device %d", ctx->device);
        }
    }
    const drt_context::Adaptive before = ctx->ad;
    MapMade made;
    MapReport r;
    if ((rc = map_adopt(ctx, device ? nullptr : m->targets, device ? m->targets : nullptr, m->flags, &made)) || (rc = map_report(ctx, &r)))
    {
        const std::string keep = g_last_error;
        (void)hipStreamSynchronize(ctx->stream);
        map_drop(ctx, made);
        ctx->ad = before;
        g_last_error = keep;
        return rc;
    }
    if ((rc = map_accept(ctx)) || (rc = map_first_list(ctx))) return rc;
    while (ctx->sm_bits)
    {
        if ((rc = map_enqueue_round(ctx))) return rc;
        if ((rc = map_finish_round(ctx))) return rc;
    }
    map_fill(m, r);
    return 0;
}

/* every device its own rows of the map and its own rounds, side by side; all the checks, the adoption included, before any renders */
extern "C" int drt_group_render_sample_map(drt_group *g, drt_sample_map *m)
{
    g_last_error.clear();
    if (!g || !m) return fail(-1, "null argument");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = map_check(c, m, true))) return rc;
    const size_t n = g->ctx.size();
    std::vector<drt_context::Adaptive> before;
    for (drt_context *c : g->ctx) before.push_back(c ? c->ad : drt_context::Adaptive{});
    std::vector<MapMade> made(n);
    auto refuse = [&](int code)
    {
        const std::string keep = g_last_error;
        for (size_t k = 0; k < n; k += 1)
            if (drt_context *c = g->ctx[k])
            {
                (void)hipSetDevice(c->device);
                (void)hipStreamSynchronize(c->stream);
                map_drop(c, made[k]);
                c->ad = before[k];
            }
        g_last_error = keep;
        return code;
    };
    /* device k of n holds rows k, k + n, ... of the tile: its targets contiguously, in a vector that lives until the reports are in */
    std::vector<std::vector<uint32_t>> rows(n);
    for (size_t k = 0; k < n; k += 1)
    {
        drt_context *c = g->ctx[k];
        if (!c) continue;
        rows[k].resize((size_t)g->rows[k] * g->tile_w);
        for (uint32_t r = 0; r < g->rows[k]; r += 1)
            memcpy(rows[k].data() + (size_t)r * g->tile_w, m->targets + ((size_t)r * n + k) * g->tile_w, (size_t)g->tile_w * sizeof(uint32_t));
        if ((rc = map_adopt(c, rows[k].data(), nullptr, m->flags, &made[k]))) return refuse(rc);
    }
    MapReport r;
    for (drt_context *c : g->ctx)
        if (c && (rc = map_report(c, &r))) return refuse(rc);
    for (drt_context *c : g->ctx)
        if (c && (rc = map_accept(c))) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = map_first_list(c))) return rc;
    std::vector<char> running(n, 0);
    for (;;)
    {
        bool any = false;
        for (size_t k = 0; k < n; k += 1)
        {
            running[k] = g->ctx[k] && g->ctx[k]->sm_bits;
            if (running[k] && (rc = map_enqueue_round(g->ctx[k]))) return rc;
            any = any || running[k];
        }
        if (!any) break;
        for (size_t k = 0; k < n; k += 1)
            if (running[k] && (rc = map_finish_round(g->ctx[k]))) return rc;
    }
    map_fill(m, r);
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* Depth-cut films (the kernel in drt_depth_kernels.h)                        */

/* what a bind is refused for, before any device call; n == 0 (the unbind) passes on any context */
static int depth_cuts_check(const drt_context *ctx, const uint32_t *depths, uint32_t n, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (n == 0) return 0;
    if (!depths) return fail(-1, "%s: null depths", name);
    if (n > DRT_MAX_DEPTH_CUTS) return fail(-1, "%s: %u cuts, at most %u", name, n, (unsigned)DRT_MAX_DEPTH_CUTS);
    for (uint32_t c = 0; c < n; c += 1)
    {
        if (depths[c] == 0 || depths[c] > ctx->params.max_depth)
            return fail(-1, "%s: cut %u has depth %u, not in 1..max_depth = %u", name, c, depths[c], ctx->params.max_depth);
        if (c > 0 && depths[c] <= depths[c - 1]) return fail(-1, "%s: the depths are not strictly ascending (cut %u: %u after %u)", name, c, depths[c], depths[c - 1]);
    }
    if (ctx->n_sensor) return fail(-4, "%s: a sensor is bound, and the two passes share a work queue: drt_bind_sensor(ctx, NULL, 0) first", name);
    if (ctx->n_buckets) return fail(-4, "%s: buckets are bound, and the two passes share a work queue: drt_bind_buckets(ctx, 0) first", name);
    if (ctx->n_lobes) return fail(-4, "%s: lobes are bound, and the two passes share a work queue: drt_bind_lobes(ctx, 0, NULL) first", name);
    if (ctx->xyz_mode) return fail(-4, "%s: the cut films are spectral films: DRT_MODE_XYZ keeps none", name);
    if (ctx->adaptive_done) return fail(-7, "%s: the film holds an adaptive render: drt_reset_film first", name);
    if (ctx->film_used) return fail(-7, "%s: the film already holds samples the cut films would lack: drt_reset_film first", name);
    return 0;
}

/* n zero-filled cut films for ctx, into `out`; the context is not touched */
static int depth_cuts_alloc(drt_context *ctx, uint32_t n, drt_context::CutFilms *out)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t S = ctx->dsc.S, n_pix = ctx->n_pix;
    for (uint32_t c = 0; c < n; c += 1)
    {
        hipError_t e = out->pixels[c].need(n_pix * (S + 1));
        if (e == hipSuccess) e = out->avgs[c].need(n_pix * S);
        if (e == hipSuccess) e = out->vars[c].need(n_pix * S);
        if (e != hipSuccess)
        {
            (void)hipGetLastError();
            return fail(-3, "drt_bind_depth_cuts: no memory for cut film %u of %u (%zu bytes each): %s", c, n, n_pix * (3 * S + 1) * 8, hipGetErrorString(e));
        }
        HIP_TRY(hipMemsetAsync(out->pixels[c], 0, n_pix * (S + 1) * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->avgs[c], 0, n_pix * S * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->vars[c], 0, n_pix * S * 8, ctx->stream));
    }
    if (n)
    {
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, depth_kernel(n, ctx->spds_in_lds), DEPTH_BLOCK, depth_lds_bytes(ctx)));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
        ctx->depth_grid_cap = std::max(1, prop.multiProcessorCount * std::max(1, per_cu)); /* (read only while cuts are bound, and set anew by every bind) */
    }
    return 0;
}

/* the stream idle, then the new films in place of the old (n == 0: none) */
static int depth_cuts_commit(drt_context *ctx, const uint32_t *depths, uint32_t n, drt_context::CutFilms *films)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->cuts = std::move(*films);
    ctx->n_cuts = n;
    for (uint32_t c = 0; c < DRT_MAX_DEPTH_CUTS; c += 1) ctx->cut_depth[c] = c < n ? depths[c] : 0;
    return 0;
}

extern "C" int drt_bind_depth_cuts(drt_context *ctx, const uint32_t *depths, uint32_t n)
{
    g_last_error.clear();
    int rc = depth_cuts_check(ctx, depths, n, "drt_bind_depth_cuts");
    if (rc) return rc;
    drt_context::CutFilms films;
    if ((rc = depth_cuts_alloc(ctx, n, &films))) return rc;
    return depth_cuts_commit(ctx, depths, n, &films);
}

static int depth_cut_index(const drt_context *ctx, uint32_t cut, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (ctx->n_cuts == 0) return fail(-4, "%s: no depth cuts are bound (drt_bind_depth_cuts)", name);
    if (cut >= ctx->n_cuts) return fail(-1, "%s: cut %u of %u", name, cut, ctx->n_cuts);
    return 0;
}

extern "C" int drt_depth_film_device_ptrs(drt_context *ctx, uint32_t cut, void **d_pixels, void **d_avgs, void **d_vars)
{
    int rc = depth_cut_index(ctx, cut, "drt_depth_film_device_ptrs");
    if (rc) return rc;
    if (d_pixels) *d_pixels = ctx->cuts.pixels[cut].get();
    if (d_avgs) *d_avgs = ctx->cuts.avgs[cut].get();
    if (d_vars) *d_vars = ctx->cuts.vars[cut].get();
    return 0;
}

extern "C" int drt_read_depth_film(drt_context *ctx, uint32_t cut, double *pixels, double *avgs, double *vars)
{
    int rc = depth_cut_index(ctx, cut, "drt_read_depth_film");
    if (rc) return rc;
    if ((rc = drt_synchronize(ctx))) return rc;
    const size_t S = ctx->dsc.S;
    if (pixels) HIP_TRY(hipMemcpy(pixels, ctx->cuts.pixels[cut], (size_t)ctx->n_pix * (S + 1) * 8, hipMemcpyDeviceToHost));
    if (avgs) HIP_TRY(hipMemcpy(avgs, ctx->cuts.avgs[cut], (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    if (vars) HIP_TRY(hipMemcpy(vars, ctx->cuts.vars[cut], (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_depth_xyz(drt_context *ctx, uint32_t cut, double *xyz)
{
    int rc = depth_cut_index(ctx, cut, "drt_read_depth_xyz");
    if (rc) return rc;
    if (!xyz) return fail(-1, "drt_read_depth_xyz: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = drt_synchronize(ctx))) return rc; /* the complete films first (see drt_read_xyz) */
    HIP_TRY(ctx->d_xyz.need((size_t)ctx->n_pix * 3));
    const uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_film_xyz_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y, ctx->cmf_z,
                       ctx->interval, ctx->n_pix, ctx->cuts.pixels[cut].get(), ctx->d_xyz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(xyz, ctx->d_xyz, (size_t)ctx->n_pix * 3 * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_depth_bgra(drt_context *ctx, uint32_t cut, int which, uint8_t *bgra)
{
    int rc = depth_cut_index(ctx, cut, "drt_read_depth_bgra");
    if (rc) return rc;
    if (!bgra) return fail(-1, "drt_read_depth_bgra: null argument");
    if (which < 0 || which > 2) return fail(-1, "which = %d: 0 sum, 1 mean, 2 variance", which);
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = drt_synchronize(ctx))) return rc;
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    const double *film = which == 0 ? ctx->cuts.pixels[cut].get() : which == 1 ? ctx->cuts.avgs[cut].get() : ctx->cuts.vars[cut].get();
    const uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_film_bgra_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y, ctx->cmf_z,
                       ctx->interval, ctx->n_pix, film, which, ctx->d_bgra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_group_bind_depth_cuts(drt_group *g, const uint32_t *depths, uint32_t n)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_bind_depth_cuts: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = depth_cuts_check(c, depths, n, "drt_group_bind_depth_cuts"))) return rc;
    std::vector<drt_context::CutFilms> films(g->ctx.size());
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = depth_cuts_alloc(g->ctx[k], n, &films[k]))) return rc; /* (what was allocated so far is released with `films`) */
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = depth_cuts_commit(g->ctx[k], depths, n, &films[k]))) return rc;
    return 0;
}

extern "C" int drt_group_read_depth_film(drt_group *g, uint32_t cut, double *pixels, double *avgs, double *vars)
{
    if (!g) return fail(-1, "drt_group_read_depth_film: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = depth_cut_index(c, cut, "drt_group_read_depth_film"))) return rc;
    if ((rc = drt_group_synchronize(g))) return rc;
    /* as group_move_rows: device k holds rows k, k + n, ... of the tile */
    const size_t n = g->ctx.size();
    double *host[3] = {pixels, avgs, vars};
    for (int f = 0; f < 3; f += 1)
    {
        if (!host[f]) continue;
        const size_t row_bytes = (size_t)g->tile_w * (f == 0 ? (size_t)g->S + 1 : (size_t)g->S) * 8;
        for (size_t k = 0; k < n; k += 1)
        {
            drt_context *c = g->ctx[k];
            if (!c) continue;
            HIP_TRY(hipSetDevice(c->device));
            const double *dev = f == 0 ? c->cuts.pixels[cut].get() : f == 1 ? c->cuts.avgs[cut].get() : c->cuts.vars[cut].get();
            HIP_TRY(hipMemcpy2D((char *)host[f] + k * row_bytes, n * row_bytes, dev, row_bytes, row_bytes, g->rows[k], hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* Sensor films (the kernel in drt_sensor_kernels.h)                          */

/* what a bind is refused for, before any device call; n == 0 (the unbind) passes on any context */
static int sensor_check(const drt_context *ctx, const double *curves, uint32_t n, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (n == 0) return 0;
    if (n > DRT_MAX_SENSOR_CHANNELS) return fail(-1, "%s: %u channels, at most %u", name, n, (unsigned)DRT_MAX_SENSOR_CHANNELS);
    if (!curves) return fail(-1, "%s: null curves", name);
    const size_t S = ctx->dsc.S;
    for (size_t i = 0; i < (size_t)n * S; i += 1)
        if (!std::isfinite(curves[i])) return fail(-1, "%s: curve %zu is not finite at wavelength %zu", name, i / S, i % S);
    if (ctx->xyz_mode) return fail(-4, "%s: the sensor film is made from the spectral film's samples: DRT_MODE_XYZ keeps none", name);
    if (ctx->n_cuts) return fail(-4, "%s: depth cuts are bound, and the two passes share a work queue: drt_bind_depth_cuts(ctx, NULL, 0) first", name);
    if (ctx->n_buckets) return fail(-4, "%s: buckets are bound, and the two passes share a work queue: drt_bind_buckets(ctx, 0) first", name);
    if (ctx->n_lobes) return fail(-4, "%s: lobes are bound, and the two passes share a work queue: drt_bind_lobes(ctx, 0, NULL) first", name);
    if (ctx->adaptive_done) return fail(-7, "%s: the film holds an adaptive render or a sample map: drt_reset_film first", name);
    if (ctx->film_used) return fail(-7, "%s: the film already holds samples the sensor film would lack: drt_reset_film first", name);
    return 0;
}

/* the curves and a zero-filled film of n channels for ctx, into `out`; the context is not touched */
static int sensor_alloc(drt_context *ctx, const double *curves, uint32_t n, drt_context::SensorFilm *out)
{
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t S = ctx->dsc.S, n_pix = ctx->n_pix;
    hipError_t e = out->curves.need((size_t)n * S);
    if (e == hipSuccess) e = out->pixels.need(n_pix * (n + 1));
    if (e == hipSuccess) e = out->avgs.need(n_pix * n);
    if (e == hipSuccess) e = out->vars.need(n_pix * n);
    if (e != hipSuccess)
    {
        (void)hipGetLastError();
        return fail(-3, "drt_bind_sensor: no memory for a sensor film of %u channels (%zu bytes): %s", n, n_pix * (3 * (size_t)n + 1) * 8, hipGetErrorString(e));
    }
    HIP_TRY(hipMemcpyAsync(out->curves, curves, (size_t)n * S * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(out->pixels, 0, n_pix * (n + 1) * 8, ctx->stream));
    HIP_TRY(hipMemsetAsync(out->avgs, 0, n_pix * n * 8, ctx->stream));
    HIP_TRY(hipMemsetAsync(out->vars, 0, n_pix * n * 8, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); /* `curves` is the caller's, and pageable */
    /* the SPD table beside the curves in LDS where the main pass keeps it there and both fit the 64 KiB a block may ask for */
    out->spds_in_lds = ctx->spds_in_lds && sensor_lds_bytes(ctx, n, true) <= 65536;
    if (sensor_lds_bytes(ctx, n, out->spds_in_lds) > 65536)
        return fail(-4, "drt_bind_sensor: %u curves of %zu wavelengths do not fit the kernel's 64 KiB of LDS", n, S);
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sensor_kernel(out->spds_in_lds), SENSOR_BLOCK, sensor_lds_bytes(ctx, n, out->spds_in_lds)));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    out->grid_cap = std::max(1, prop.multiProcessorCount * std::max(1, per_cu));
    return 0;
}

/* the stream idle, then the new film in place of the old (n == 0: none) */
static int sensor_commit(drt_context *ctx, uint32_t n, drt_context::SensorFilm *film)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->sensor = std::move(*film);
    ctx->n_sensor = n;
    return 0;
}

extern "C" int drt_bind_sensor(drt_context *ctx, const double *curves, uint32_t n)
{
    g_last_error.clear();
    int rc = sensor_check(ctx, curves, n, "drt_bind_sensor");
    if (rc) return rc;
    drt_context::SensorFilm film;
    if ((rc = sensor_alloc(ctx, curves, n, &film))) return rc;
    return sensor_commit(ctx, n, &film);
}

static int sensor_bound(const drt_context *ctx, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (ctx->n_sensor == 0) return fail(-4, "%s: no sensor is bound (drt_bind_sensor)", name);
    return 0;
}

extern "C" int drt_sensor_film_device_ptrs(drt_context *ctx, void **d_pixels, void **d_avgs, void **d_vars)
{
    int rc = sensor_bound(ctx, "drt_sensor_film_device_ptrs");
    if (rc) return rc;
    if (d_pixels) *d_pixels = ctx->sensor.pixels.get();
    if (d_avgs) *d_avgs = ctx->sensor.avgs.get();
    if (d_vars) *d_vars = ctx->sensor.vars.get();
    return 0;
}

extern "C" int drt_read_sensor_film(drt_context *ctx, double *pixels, double *avgs, double *vars)
{
    int rc = sensor_bound(ctx, "drt_read_sensor_film");
    if (rc) return rc;
    if ((rc = drt_synchronize(ctx))) return rc;
    const size_t n = ctx->n_sensor;
    if (pixels) HIP_TRY(hipMemcpy(pixels, ctx->sensor.pixels, (size_t)ctx->n_pix * (n + 1) * 8, hipMemcpyDeviceToHost));
    if (avgs) HIP_TRY(hipMemcpy(avgs, ctx->sensor.avgs, (size_t)ctx->n_pix * n * 8, hipMemcpyDeviceToHost));
    if (vars) HIP_TRY(hipMemcpy(vars, ctx->sensor.vars, (size_t)ctx->n_pix * n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_sensor_bgra(drt_context *ctx, int which, const double *matrix, uint8_t *bgra)
{
    int rc = sensor_bound(ctx, "drt_read_sensor_bgra");
    if (rc) return rc;
    if (!matrix || !bgra) return fail(-1, "drt_read_sensor_bgra: null argument");
    if (which < 0 || which > 1) return fail(-1, "which = %d: 0 sum / filter, 1 mean", which);
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = drt_synchronize(ctx))) return rc;
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    SensorMatrix m{};
    for (uint32_t i = 0; i < 3 * ctx->n_sensor; i += 1) m.m[i / ctx->n_sensor][i % ctx->n_sensor] = matrix[i];
    const uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_sensor_bgra_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->n_pix, ctx->n_sensor,
                       which == 0 ? ctx->sensor.pixels.get() : ctx->sensor.avgs.get(), which, m, ctx->d_bgra.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_group_bind_sensor(drt_group *g, const double *curves, uint32_t n)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_bind_sensor: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = sensor_check(c, curves, n, "drt_group_bind_sensor"))) return rc;
    std::vector<drt_context::SensorFilm> films(g->ctx.size());
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = sensor_alloc(g->ctx[k], curves, n, &films[k]))) return rc; /* (what was allocated so far is released with `films`) */
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = sensor_commit(g->ctx[k], n, &films[k]))) return rc;
    return 0;
}

extern "C" int drt_group_read_sensor_film(drt_group *g, double *pixels, double *avgs, double *vars)
{
    if (!g) return fail(-1, "drt_group_read_sensor_film: null group");
    int rc = 0;
    uint32_t ch = 0;
    for (drt_context *c : g->ctx)
    {
        if (c && (rc = sensor_bound(c, "drt_group_read_sensor_film"))) return rc;
        if (c) ch = c->n_sensor;
    }
    if ((rc = drt_group_synchronize(g))) return rc;
    /* as group_move_rows: device k holds rows k, k + n, ... of the tile */
    const size_t n = g->ctx.size();
    double *host[3] = {pixels, avgs, vars};
    for (int f = 0; f < 3; f += 1)
    {
        if (!host[f]) continue;
        const size_t row_bytes = (size_t)g->tile_w * (f == 0 ? (size_t)ch + 1 : (size_t)ch) * 8;
        for (size_t k = 0; k < n; k += 1)
        {
            drt_context *c = g->ctx[k];
            if (!c) continue;
            HIP_TRY(hipSetDevice(c->device));
            const double *dev = f == 0 ? c->sensor.pixels.get() : f == 1 ? c->sensor.avgs.get() : c->sensor.vars.get();
            HIP_TRY(hipMemcpy2D((char *)host[f] + k * row_bytes, n * row_bytes, dev, row_bytes, row_bytes, g->rows[k], hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* Bucket films (the kernels in drt_bucket_kernels.h)                         */

/* what a bind is refused for, before any device call; n == 0 (the unbind) passes on any context */
static int buckets_check(const drt_context *ctx, uint32_t n, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (n == 0) return 0;
    if (n > DRT_MAX_BUCKETS) return fail(-1, "%s: %u buckets, at most %u", name, n, (unsigned)DRT_MAX_BUCKETS);
    if (ctx->xyz_mode) return fail(-4, "%s: the bucket films are spectral films: DRT_MODE_XYZ keeps none", name);
    if (ctx->n_cuts) return fail(-4, "%s: depth cuts are bound, and the two passes share a work queue: drt_bind_depth_cuts(ctx, NULL, 0) first", name);
    if (ctx->n_sensor) return fail(-4, "%s: a sensor is bound, and the two passes share a work queue: drt_bind_sensor(ctx, NULL, 0) first", name);
    if (ctx->n_lobes) return fail(-4, "%s: lobes are bound, and the two passes share a work queue: drt_bind_lobes(ctx, 0, NULL) first", name);
    if (ctx->adaptive_done) return fail(-7, "%s: the film holds an adaptive render or a sample map: drt_reset_film first", name);
    if (ctx->film_used) return fail(-7, "%s: the film already holds samples the bucket films would lack: drt_reset_film first", name);
    return 0;
}

/* n zero-filled bucket films for ctx, into `out`; the context is not touched */
static int buckets_alloc(drt_context *ctx, uint32_t n, drt_context::BucketFilms *out)
{
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t S = ctx->dsc.S, n_pix = ctx->n_pix;
    for (uint32_t b = 0; b < n; b += 1)
    {
        hipError_t e = out->pixels[b].need(n_pix * (S + 1));
        if (e == hipSuccess) e = out->avgs[b].need(n_pix * S);
        if (e == hipSuccess) e = out->vars[b].need(n_pix * S);
        if (e != hipSuccess)
        {
            (void)hipGetLastError();
            return fail(-3, "drt_bind_buckets: no memory for bucket film %u of %u (%zu bytes each): %s", b, n, n_pix * (3 * S + 1) * 8, hipGetErrorString(e));
        }
        HIP_TRY(hipMemsetAsync(out->pixels[b], 0, n_pix * (S + 1) * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->avgs[b], 0, n_pix * S * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->vars[b], 0, n_pix * S * 8, ctx->stream));
    }
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bucket_kernel(n, ctx->spds_in_lds), BUCKET_BLOCK, depth_lds_bytes(ctx)));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    out->grid_cap = std::max(1, prop.multiProcessorCount * std::max(1, per_cu));
    return 0;
}

/* the stream idle, then the new films in place of the old (n == 0: none); an earlier resolve's results go with the old films */
static int buckets_commit(drt_context *ctx, uint32_t n, drt_context::BucketFilms *films)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->buckets = std::move(*films);
    ctx->n_buckets = n;
    ctx->bk_samples = 0;
    ctx->bk_valid = false;
    ctx->d_bk_estimate = DevBuf<double>();
    ctx->d_bk_error = DevBuf<double>();
    ctx->d_bk_packed = DevBuf<double>();
    return 0;
}

extern "C" int drt_bind_buckets(drt_context *ctx, uint32_t n)
{
    g_last_error.clear();
    int rc = buckets_check(ctx, n, "drt_bind_buckets");
    if (rc) return rc;
    drt_context::BucketFilms films;
    if ((rc = buckets_alloc(ctx, n, &films))) return rc;
    return buckets_commit(ctx, n, &films);
}

static int bucket_index(const drt_context *ctx, uint32_t b, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (ctx->n_buckets == 0) return fail(-4, "%s: no buckets are bound (drt_bind_buckets)", name);
    if (b >= ctx->n_buckets) return fail(-1, "%s: bucket %u of %u", name, b, ctx->n_buckets);
    return 0;
}

extern "C" int drt_bucket_film_device_ptrs(drt_context *ctx, uint32_t b, void **d_pixels, void **d_avgs, void **d_vars)
{
    int rc = bucket_index(ctx, b, "drt_bucket_film_device_ptrs");
    if (rc) return rc;
    if ((rc = drt_synchronize(ctx))) return rc; /* (a launch that ran out of records is rendered again before anyone reads the films) */
    if (d_pixels) *d_pixels = ctx->buckets.pixels[b].get();
    if (d_avgs) *d_avgs = ctx->buckets.avgs[b].get();
    if (d_vars) *d_vars = ctx->buckets.vars[b].get();
    return 0;
}

extern "C" int drt_read_bucket_film(drt_context *ctx, uint32_t b, double *pixels, double *avgs, double *vars)
{
    int rc = bucket_index(ctx, b, "drt_read_bucket_film");
    if (rc) return rc;
    if ((rc = drt_synchronize(ctx))) return rc;
    const size_t S = ctx->dsc.S;
    if (pixels) HIP_TRY(hipMemcpy(pixels, ctx->buckets.pixels[b], (size_t)ctx->n_pix * (S + 1) * 8, hipMemcpyDeviceToHost));
    if (avgs) HIP_TRY(hipMemcpy(avgs, ctx->buckets.avgs[b], (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    if (vars) HIP_TRY(hipMemcpy(vars, ctx->buckets.vars[b], (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    return 0;
}

/* what a resolve is refused for, before any device call */
static int resolve_check(const drt_context *ctx, uint32_t trim, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (ctx->n_buckets == 0) return fail(-4, "%s: no buckets are bound (drt_bind_buckets)", name);
    if (ctx->n_buckets < 2) return fail(-4, "%s: one bucket has no scatter to resolve: bind at least 2", name);
    if (2ull * trim >= ctx->n_buckets) return fail(-1, "%s: trim = %u leaves nothing of %u buckets (2 * trim < n)", name, trim, ctx->n_buckets);
    if (ctx->bk_samples < ctx->n_buckets)
        return fail(-7, "%s: the film holds %llu samples, fewer than its %u buckets: some bucket is empty", name, (unsigned long long)ctx->bk_samples, ctx->n_buckets);
    return 0;
}

template <int NB>
static void launch_resolve(drt_context *ctx, uint64_t n_values, const BucketMeans &means, uint32_t trim)
{
    hipLaunchKernelGGL(drt_bucket_resolve_kernel<NB>, dim3((uint32_t)((n_values + 255) / 256)), dim3(256), 0, ctx->stream, n_values, means, trim,
                       ctx->d_bk_estimate.get(), ctx->d_bk_error.get());
}

static int resolve_enqueue(drt_context *ctx, uint32_t trim)
{
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = drt_synchronize(ctx); /* the complete films first (see drt_read_xyz) */
    if (rc) return rc;
    const uint64_t n_values = ctx->n_pix * (uint64_t)ctx->dsc.S;
    if ((n_values + 255) / 256 > 0x7FFFFFFFull) return fail(-1, "drt_resolve_buckets: tile too large for one launch");
    ctx->bk_valid = false;
    hipError_t e = ctx->d_bk_estimate.need(n_values);
    if (e == hipSuccess) e = ctx->d_bk_error.need(n_values);
    if (e != hipSuccess)
    {
        (void)hipGetLastError();
        return fail(-3, "drt_resolve_buckets: no memory for the estimate and the error (%llu bytes each): %s", (unsigned long long)n_values * 8, hipGetErrorString(e));
    }
    BucketMeans means{};
    for (uint32_t b = 0; b < ctx->n_buckets; b += 1) means.avgs[b] = ctx->buckets.avgs[b].get();
    switch (ctx->n_buckets)
    {
        case 2: launch_resolve<2>(ctx, n_values, means, trim); break;
        case 3: launch_resolve<3>(ctx, n_values, means, trim); break;
        case 4: launch_resolve<4>(ctx, n_values, means, trim); break;
        case 5: launch_resolve<5>(ctx, n_values, means, trim); break;
        case 6: launch_resolve<6>(ctx, n_values, means, trim); break;
        case 7: launch_resolve<7>(ctx, n_values, means, trim); break;
        default: launch_resolve<8>(ctx, n_values, means, trim); break;
    }
    HIP_TRY(hipGetLastError());
    ctx->bk_valid = true;
    ctx->bk_gen = ctx->film_gen;
    return 0;
}

extern "C" int drt_resolve_buckets(drt_context *ctx, uint32_t trim)
{
    g_last_error.clear();
    int rc = resolve_check(ctx, trim, "drt_resolve_buckets");
    if (rc) return rc;
    return resolve_enqueue(ctx, trim);
}

static int resolve_current(const drt_context *ctx, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (ctx->n_buckets == 0) return fail(-4, "%s: no buckets are bound (drt_bind_buckets)", name);
    if (!ctx->bk_valid) return fail(-7, "%s: nothing is resolved yet: drt_resolve_buckets first", name);
    if (ctx->bk_gen != ctx->film_gen) return fail(-7, "%s: the film has changed since the last resolve: drt_resolve_buckets again", name);
    return 0;
}

extern "C" int drt_bucket_resolve_device_ptrs(drt_context *ctx, void **d_estimate, void **d_error)
{
    int rc = resolve_current(ctx, "drt_bucket_resolve_device_ptrs");
    if (rc) return rc;
    if (d_estimate) *d_estimate = ctx->d_bk_estimate.get();
    if (d_error) *d_error = ctx->d_bk_error.get();
    return 0;
}

extern "C" int drt_read_bucket_resolve(drt_context *ctx, double *estimate, double *error)
{
    int rc = resolve_current(ctx, "drt_read_bucket_resolve");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t bytes = (size_t)ctx->n_pix * ctx->dsc.S * 8;
    if (estimate) HIP_TRY(hipMemcpy(estimate, ctx->d_bk_estimate, bytes, hipMemcpyDeviceToHost));
    if (error) HIP_TRY(hipMemcpy(error, ctx->d_bk_error, bytes, hipMemcpyDeviceToHost));
    return 0;
}

/* drt_film_xyz_kernel reads [n_pix][S + 1] and divides by the last column: the estimate with a column of 1.0 (x / 1.0 is x) */
extern "C" int drt_read_bucket_resolve_xyz(drt_context *ctx, double *xyz)
{
    int rc = resolve_current(ctx, "drt_read_bucket_resolve_xyz");
    if (rc) return rc;
    if (!xyz) return fail(-1, "drt_read_bucket_resolve_xyz: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t S = ctx->dsc.S;
    HIP_TRY(ctx->d_xyz.need((size_t)ctx->n_pix * 3));
    HIP_TRY(ctx->d_bk_packed.need((size_t)ctx->n_pix * (S + 1)));
    const uint64_t n_values = ctx->n_pix * (uint64_t)(S + 1);
    hipLaunchKernelGGL(drt_bucket_pack_kernel, dim3((uint32_t)((n_values + 255) / 256)), dim3(256), 0, ctx->stream, n_values, (uint32_t)S,
                       (const double *)ctx->d_bk_estimate.get(), ctx->d_bk_packed.get());
    HIP_TRY(hipGetLastError());
    const uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_film_xyz_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y, ctx->cmf_z,
                       ctx->interval, ctx->n_pix, (const double *)ctx->d_bk_packed.get(), ctx->d_xyz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(xyz, ctx->d_xyz, (size_t)ctx->n_pix * 3 * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_bucket_resolve_bgra(drt_context *ctx, uint8_t *bgra)
{
    int rc = resolve_current(ctx, "drt_read_bucket_resolve_bgra");
    if (rc) return rc;
    if (!bgra) return fail(-1, "drt_read_bucket_resolve_bgra: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    const uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_film_bgra_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y, ctx->cmf_z,
                       ctx->interval, ctx->n_pix, (const double *)ctx->d_bk_estimate.get(), 1, ctx->d_bgra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_group_bind_buckets(drt_group *g, uint32_t n)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_bind_buckets: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = buckets_check(c, n, "drt_group_bind_buckets"))) return rc;
    std::vector<drt_context::BucketFilms> films(g->ctx.size());
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = buckets_alloc(g->ctx[k], n, &films[k]))) return rc; /* (what was allocated so far is released with `films`) */
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = buckets_commit(g->ctx[k], n, &films[k]))) return rc;
    return 0;
}

/* as group_move_rows: device k of n holds rows k, k + n, ... of the tile; dev(c): that context's buffer, rows of row_bytes bytes */
template <typename F>
static int group_gather_bucket_rows(drt_group *g, double *host, size_t row_bytes, F dev)
{
    const size_t n = g->ctx.size();
    for (size_t k = 0; k < n; k += 1)
    {
        drt_context *c = g->ctx[k];
        if (!c) continue;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpy2D((char *)host + k * row_bytes, n * row_bytes, dev(c), row_bytes, row_bytes, g->rows[k], hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int drt_group_read_bucket_film(drt_group *g, uint32_t b, double *pixels, double *avgs, double *vars)
{
    if (!g) return fail(-1, "drt_group_read_bucket_film: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = bucket_index(c, b, "drt_group_read_bucket_film"))) return rc;
    if ((rc = drt_group_synchronize(g))) return rc;
    double *host[3] = {pixels, avgs, vars};
    for (int f = 0; f < 3; f += 1)
    {
        if (!host[f]) continue;
        const size_t row_bytes = (size_t)g->tile_w * (f == 0 ? (size_t)g->S + 1 : (size_t)g->S) * 8;
        rc = group_gather_bucket_rows(g, host[f], row_bytes, [&](drt_context *c) -> const double * {
            return f == 0 ? c->buckets.pixels[b].get() : f == 1 ? c->buckets.avgs[b].get() : c->buckets.vars[b].get();
        });
        if (rc) return rc;
    }
    return 0;
}

extern "C" int drt_group_resolve_buckets(drt_group *g, uint32_t trim)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_resolve_buckets: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = resolve_check(c, trim, "drt_group_resolve_buckets"))) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = resolve_enqueue(c, trim))) return rc;
    return 0;
}

extern "C" int drt_group_read_bucket_resolve(drt_group *g, double *estimate, double *error)
{
    if (!g) return fail(-1, "drt_group_read_bucket_resolve: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = resolve_current(c, "drt_group_read_bucket_resolve"))) return rc;
    for (drt_context *c : g->ctx)
        if (c)
        {
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    const size_t row_bytes = (size_t)g->tile_w * (size_t)g->S * 8;
    if (estimate && (rc = group_gather_bucket_rows(g, estimate, row_bytes, [](drt_context *c) -> const double * { return c->d_bk_estimate.get(); }))) return rc;
    if (error && (rc = group_gather_bucket_rows(g, error, row_bytes, [](drt_context *c) -> const double * { return c->d_bk_error.get(); }))) return rc;
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* Lobe films (the kernel in drt_lobe_kernels.h)                              */

/* what a bind is refused for, before any device call; n == 0 (the unbind) passes on any context */
static int lobes_check(const drt_context *ctx, uint32_t n, const drt_lobe_map *map, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (n == 0) return 0;
    if (n > DRT_MAX_LOBE_FILMS) return fail(-1, "%s: %u films, at most %u", name, n, (unsigned)DRT_MAX_LOBE_FILMS);
    if (!map) return fail(-1, "%s: null map", name);
    if (map->emission >= n && map->emission != DRT_LOBE_NONE) return fail(-1, "%s: the map sends emission to film %u of %u", name, (unsigned)map->emission, n);
    for (uint32_t f = 0; f < (uint32_t)DRT_NUM_BDSFS; f += 1)
    {
        if (map->direct[f] >= n && map->direct[f] != DRT_LOBE_NONE)
            return fail(-1, "%s: the map sends the direct light of function %u to film %u of %u", name, f, (unsigned)map->direct[f], n);
        if (map->indirect[f] >= n && map->indirect[f] != DRT_LOBE_NONE)
            return fail(-1, "%s: the map sends the indirect light of function %u to film %u of %u", name, f, (unsigned)map->indirect[f], n);
    }
    if (ctx->xyz_mode) return fail(-4, "%s: the lobe films are spectral films: DRT_MODE_XYZ keeps none", name);
    if (ctx->n_cuts) return fail(-4, "%s: depth cuts are bound, and the two passes share a work queue: drt_bind_depth_cuts(ctx, NULL, 0) first", name);
    if (ctx->n_sensor) return fail(-4, "%s: a sensor is bound, and the two passes share a work queue: drt_bind_sensor(ctx, NULL, 0) first", name);
    if (ctx->n_buckets) return fail(-4, "%s: buckets are bound, and the two passes share a work queue: drt_bind_buckets(ctx, 0) first", name);
    if (ctx->adaptive_done) return fail(-7, "%s: the film holds an adaptive render or a sample map: drt_reset_film first", name);
    if (ctx->film_used) return fail(-7, "%s: the film already holds samples the lobe films would lack: drt_reset_film first", name);
    return 0;
}

/* n zero-filled lobe films for ctx, into `out`; the context is not touched */
static int lobes_alloc(drt_context *ctx, uint32_t n, drt_context::LobeFilms *out)
{
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t S = ctx->dsc.S, n_pix = ctx->n_pix;
    for (uint32_t c = 0; c < n; c += 1)
    {
        hipError_t e = out->pixels[c].need(n_pix * (S + 1));
        if (e == hipSuccess) e = out->avgs[c].need(n_pix * S);
        if (e == hipSuccess) e = out->vars[c].need(n_pix * S);
        if (e != hipSuccess)
        {
            (void)hipGetLastError();
            return fail(-3, "drt_bind_lobes: no memory for lobe film %u of %u (%zu bytes each): %s", c, n, n_pix * (3 * S + 1) * 8, hipGetErrorString(e));
        }
        HIP_TRY(hipMemsetAsync(out->pixels[c], 0, n_pix * (S + 1) * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->avgs[c], 0, n_pix * S * 8, ctx->stream));
        HIP_TRY(hipMemsetAsync(out->vars[c], 0, n_pix * S * 8, ctx->stream));
    }
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lobe_kernel(n, ctx->spds_in_lds), LOBE_BLOCK, depth_lds_bytes(ctx)));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    out->grid_cap = std::max(1, prop.multiProcessorCount * std::max(1, per_cu));
    return 0;
}

/* the stream idle, then the new films and the map in place of the old (n == 0: none) */
static int lobes_commit(drt_context *ctx, uint32_t n, const drt_lobe_map *map, drt_context::LobeFilms *films)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->lobes = std::move(*films);
    ctx->n_lobes = n;
    ctx->lobe_map = n ? *map : drt_lobe_map{};
    return 0;
}

extern "C" int drt_bind_lobes(drt_context *ctx, uint32_t n, const drt_lobe_map *map)
{
    g_last_error.clear();
    int rc = lobes_check(ctx, n, map, "drt_bind_lobes");
    if (rc) return rc;
    drt_context::LobeFilms films;
    if ((rc = lobes_alloc(ctx, n, &films))) return rc;
    return lobes_commit(ctx, n, map, &films);
}

static int lobe_index(const drt_context *ctx, uint32_t c, const char *name)
{
    if (!ctx) return fail(-1, "%s: null context", name);
    if (ctx->n_lobes == 0) return fail(-4, "%s: no lobes are bound (drt_bind_lobes)", name);
    if (c >= ctx->n_lobes) return fail(-1, "%s: film %u of %u", name, c, ctx->n_lobes);
    return 0;
}

extern "C" int drt_lobe_film_device_ptrs(drt_context *ctx, uint32_t c, void **d_pixels, void **d_avgs, void **d_vars)
{
    int rc = lobe_index(ctx, c, "drt_lobe_film_device_ptrs");
    if (rc) return rc;
    if ((rc = drt_synchronize(ctx))) return rc; /* (a launch that ran out of records is rendered again before anyone reads the films) */
    if (d_pixels) *d_pixels = ctx->lobes.pixels[c].get();
    if (d_avgs) *d_avgs = ctx->lobes.avgs[c].get();
    if (d_vars) *d_vars = ctx->lobes.vars[c].get();
    return 0;
}

extern "C" int drt_read_lobe_film(drt_context *ctx, uint32_t c, double *pixels, double *avgs, double *vars)
{
    int rc = lobe_index(ctx, c, "drt_read_lobe_film");
    if (rc) return rc;
    if ((rc = drt_synchronize(ctx))) return rc;
    const size_t S = ctx->dsc.S;
    if (pixels) HIP_TRY(hipMemcpy(pixels, ctx->lobes.pixels[c], (size_t)ctx->n_pix * (S + 1) * 8, hipMemcpyDeviceToHost));
    if (avgs) HIP_TRY(hipMemcpy(avgs, ctx->lobes.avgs[c], (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    if (vars) HIP_TRY(hipMemcpy(vars, ctx->lobes.vars[c], (size_t)ctx->n_pix * S * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_lobe_xyz(drt_context *ctx, uint32_t c, double *xyz)
{
    int rc = lobe_index(ctx, c, "drt_read_lobe_xyz");
    if (rc) return rc;
    if (!xyz) return fail(-1, "drt_read_lobe_xyz: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = drt_synchronize(ctx))) return rc; /* the complete films first (see drt_read_xyz) */
    HIP_TRY(ctx->d_xyz.need((size_t)ctx->n_pix * 3));
    const uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_film_xyz_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y, ctx->cmf_z,
                       ctx->interval, ctx->n_pix, ctx->lobes.pixels[c].get(), ctx->d_xyz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(xyz, ctx->d_xyz, (size_t)ctx->n_pix * 3 * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_lobe_bgra(drt_context *ctx, uint32_t c, int which, uint8_t *bgra)
{
    int rc = lobe_index(ctx, c, "drt_read_lobe_bgra");
    if (rc) return rc;
    if (!bgra) return fail(-1, "drt_read_lobe_bgra: null argument");
    if (which < 0 || which > 2) return fail(-1, "which = %d: 0 sum, 1 mean, 2 variance", which);
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = drt_synchronize(ctx))) return rc;
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    const double *film = which == 0 ? ctx->lobes.pixels[c].get() : which == 1 ? ctx->lobes.avgs[c].get() : ctx->lobes.vars[c].get();
    const uint32_t grid = (uint32_t)((ctx->n_pix + 255) / 256);
    hipLaunchKernelGGL(drt_film_bgra_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y, ctx->cmf_z,
                       ctx->interval, ctx->n_pix, film, which, ctx->d_bgra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_group_bind_lobes(drt_group *g, uint32_t n, const drt_lobe_map *map)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_bind_lobes: null group");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = lobes_check(c, n, map, "drt_group_bind_lobes"))) return rc;
    std::vector<drt_context::LobeFilms> films(g->ctx.size());
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = lobes_alloc(g->ctx[k], n, &films[k]))) return rc; /* (what was allocated so far is released with `films`) */
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = lobes_commit(g->ctx[k], n, map, &films[k]))) return rc;
    return 0;
}

extern "C" int drt_group_read_lobe_film(drt_group *g, uint32_t c, double *pixels, double *avgs, double *vars)
{
    if (!g) return fail(-1, "drt_group_read_lobe_film: null group");
    int rc = 0;
    for (drt_context *x : g->ctx)
        if (x && (rc = lobe_index(x, c, "drt_group_read_lobe_film"))) return rc;
    if ((rc = drt_group_synchronize(g))) return rc;
    double *host[3] = {pixels, avgs, vars};
    for (int f = 0; f < 3; f += 1)
    {
        if (!host[f]) continue;
        const size_t row_bytes = (size_t)g->tile_w * (f == 0 ? (size_t)g->S + 1 : (size_t)g->S) * 8;
        rc = group_gather_bucket_rows(g, host[f], row_bytes, [&](drt_context *x) -> const double * {
            return f == 0 ? x->lobes.pixels[c].get() : f == 1 ? x->lobes.avgs[c].get() : x->lobes.vars[c].get();
        });
        if (rc) return rc;
    }
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* The variance-guided denoiser (kernels in drt_denoise_kernels.h)           */

/* the parameter ranges: no device call before these have passed */
static int denoise_check(const drt_denoise *d)
{
    if (!d) return fail(-1, "null argument");
    if (d->radius > DENOISE_MAX_RADIUS) return fail(-1, "denoise: radius = %u: from 0 to %d", d->radius, DENOISE_MAX_RADIUS);
    if (d->patch > DENOISE_MAX_PATCH) return fail(-1, "denoise: patch = %u: from 0 to %d", d->patch, DENOISE_MAX_PATCH);
    if (d->flags != 0) return fail(-1, "denoise: flags = %u: 0 (reserved)", d->flags);
    if (!std::isfinite(d->k) || !(d->k > 0.0)) return fail(-1, "denoise: k = %g: a finite number above 0", d->k);
    if (!std::isfinite(d->alpha) || !(d->alpha >= 0.0)) return fail(-1, "denoise: alpha = %g: a finite number, 0 or more", d->alpha);
    return 0;
}

static int denoise_check_film(uint32_t mode, uint32_t row_stride, uint32_t S)
{
    if (mode == DRT_MODE_XYZ) return fail(-4, "denoise: needs the spectral film (DRT_MODE_XYZ keeps no mean and no variance)");
    if (row_stride != 1) return fail(-4, "denoise: row_stride = %u: a pixel's neighbours are not in this film (row_stride must be 1; a group gathers the film, drt_group_denoise)", row_stride);
    if (S == 0 || S > DENOISE_MAX_S) return fail(-4, "denoise: %u wavelengths: from 1 to %d", S, DENOISE_MAX_S);
    return 0;
}

static size_t denoise_halo_bytes(const drt_denoise *d)
{
    const size_t side = DENOISE_TILE + 2 * (size_t)(d->radius + d->patch);
    return side * side * DENOISE_LDS_FIELDS * sizeof(double);
}

/* the three kernels on `stream`, timed; dp holds every pointer. The current device is the buffers'. */
static int denoise_enqueue(hipStream_t stream, const DenoiseParams &dp, const drt_denoise *d, double *kernel_ms)
{
    const uint64_t n_pix = (uint64_t)dp.tile_w * dp.tile_h;
    const size_t halo = denoise_halo_bytes(d);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(drt_denoise_weight_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)halo));
    Event ev[2];
    HIP_TRY(ev[0].need());
    HIP_TRY(ev[1].need());
    HIP_TRY(hipMemsetAsync(dp.unusable, 0, sizeof(uint32_t), stream));
    HIP_TRY(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(drt_denoise_guide_kernel, dim3((uint32_t)((n_pix + DENOISE_BLOCK - 1) / DENOISE_BLOCK)), dim3(DENOISE_BLOCK), 0, stream, dp);
    hipLaunchKernelGGL(drt_denoise_weight_kernel, dim3((dp.tile_w + DENOISE_TILE - 1) / DENOISE_TILE, (dp.tile_h + DENOISE_TILE - 1) / DENOISE_TILE),
                       dim3(DENOISE_TILE, DENOISE_TILE), halo, stream, dp);
    hipLaunchKernelGGL(drt_denoise_apply_kernel, dim3((dp.tile_w + DENOISE_APPLY_SIDE - 1) / DENOISE_APPLY_SIDE, (dp.tile_h + DENOISE_APPLY_SIDE - 1) / DENOISE_APPLY_SIDE),
                       dim3(DENOISE_BLOCK), 0, stream, dp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (kernel_ms) *kernel_ms = (double)ms;
    return 0;
}

static void denoise_fill(DenoiseParams *dp, const drt_denoise *d, uint32_t S, uint32_t tile_w, uint32_t tile_h, double interval)
{
    memset(dp, 0, sizeof(*dp));
    dp->S = S;
    dp->tile_w = tile_w;
    dp->tile_h = tile_h;
    dp->radius = d->radius;
    dp->patch = d->patch;
    dp->n_window = (2 * d->radius + 1) * (2 * d->radius + 1);
    dp->interval = interval;
    dp->k2 = d->k * d->k;
    dp->alpha = d->alpha;
}

extern "C" int drt_denoise_film(drt_context *ctx, drt_denoise *d)
{
    if (!ctx || !d) return fail(-1, "null argument");
    int rc = denoise_check(d);
    if (rc) return rc;
    if ((rc = denoise_check_film(ctx->xyz_mode ? DRT_MODE_XYZ : DRT_MODE_SPECTRAL, ctx->params.row_stride, ctx->dsc.S))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = drt_synchronize(ctx))) return rc; /* the complete film first (see drt_read_xyz) */
    ctx->dn_valid = false;
    const uint32_t S = ctx->dsc.S;
    const size_t n_pix = ctx->n_pix;
    DenoiseParams dp;
    denoise_fill(&dp, d, S, ctx->params.tile_w, ctx->params.tile_h, ctx->interval);
    HIP_TRY(ctx->d_dn_mean.need(n_pix * S));
    HIP_TRY(ctx->d_dn_var.need(n_pix * S));
    HIP_TRY(ctx->d_dn_guide.need(n_pix * DENOISE_GUIDE_WORDS));
    HIP_TRY(ctx->d_dn_wsum.need(n_pix));
    HIP_TRY(ctx->d_dn_unusable.need(1));
    if (ctx->dn_window_cap < dp.n_window)
    {
        ctx->dn_window_cap = 0;
        HIP_TRY(ctx->d_dn_weights.remake(n_pix * dp.n_window));
        ctx->dn_window_cap = dp.n_window;
    }
    dp.rw = ctx->dsc.spds + (size_t)ctx->cmf_rw * S;
    dp.cx = ctx->dsc.spds + (size_t)ctx->cmf_x * S;
    dp.cy = ctx->dsc.spds + (size_t)ctx->cmf_y * S;
    dp.cz = ctx->dsc.spds + (size_t)ctx->cmf_z * S;
    dp.pixels = ctx->d_pixels;
    dp.avgs = ctx->d_avgs;
    dp.vars = ctx->d_vars;
    dp.guide = ctx->d_dn_guide;
    dp.weights = ctx->d_dn_weights;
    dp.wsum = ctx->d_dn_wsum;
    dp.mean = ctx->d_dn_mean;
    dp.var = ctx->d_dn_var;
    dp.unusable = ctx->d_dn_unusable;
    if ((rc = denoise_enqueue(ctx->stream, dp, d, &d->kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(&d->unusable, ctx->d_dn_unusable, sizeof(uint32_t), hipMemcpyDeviceToHost));
    ctx->dn_gen = ctx->film_gen;
    ctx->dn_valid = true;
    return 0;
}

static int denoise_current(drt_context *ctx)
{
    if (!ctx->dn_valid) return fail(-4, "no denoised film: drt_denoise_film first");
    if (ctx->dn_gen != ctx->film_gen) return fail(-4, "the film has changed since drt_denoise_film: denoise it again");
    return 0;
}

extern "C" int drt_read_denoised(drt_context *ctx, double *mean, double *var)
{
    if (!ctx) return fail(-1, "null context");
    int rc = denoise_current(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->n_pix * ctx->dsc.S * 8;
    if (mean) HIP_TRY(hipMemcpy(mean, ctx->d_dn_mean, bytes, hipMemcpyDeviceToHost));
    if (var) HIP_TRY(hipMemcpy(var, ctx->d_dn_var, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_denoised_bgra(drt_context *ctx, uint8_t *bgra)
{
    if (!ctx || !bgra) return fail(-1, "null argument");
    int rc = denoise_current(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    /* the conversion drt_read_bgra(ctx, 1, ...) applies to the running mean, on the denoised mean */
    hipLaunchKernelGGL(drt_film_bgra_kernel, dim3((uint32_t)((ctx->n_pix + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dsc, ctx->cmf_rw, ctx->cmf_x,
                       ctx->cmf_y, ctx->cmf_z, ctx->interval, ctx->n_pix, (const double *)ctx->d_dn_mean, 1, ctx->d_bgra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

/* One-shot on host buffers of a whole film, on the current device: rows = the four colour-matching rows on that device. */
static int denoise_host_film(const double *const d_rows[4], uint32_t S, uint32_t tile_w, uint32_t tile_h, double interval, drt_denoise *d,
                             const double *pixels, const double *avgs, const double *vars, double *mean, double *var)
{
    const size_t n_pix = (size_t)tile_w * tile_h;
    DenoiseParams dp;
    denoise_fill(&dp, d, S, tile_w, tile_h, interval);
    DevBuf<double> film[3], out[2], guide, weights, wsum; /* pixels, avgs, vars; mean, var */
    DevBuf<uint32_t> unusable;
    const size_t words[3] = {n_pix * (S + 1), n_pix * S, n_pix * S};
    for (int k = 0; k < 3; k += 1) HIP_TRY(film[k].need(words[k]));
    for (int k = 0; k < 2; k += 1) HIP_TRY(out[k].need(n_pix * S));
    HIP_TRY(guide.need(n_pix * DENOISE_GUIDE_WORDS));
    HIP_TRY(weights.need(n_pix * dp.n_window));
    HIP_TRY(wsum.need(n_pix));
    HIP_TRY(unusable.need(1));
    const double *src[3] = {pixels, avgs, vars};
    for (int k = 0; k < 3; k += 1) HIP_TRY(hipMemcpy(film[k], src[k], words[k] * 8, hipMemcpyHostToDevice));
    dp.rw = d_rows[0];
    dp.cx = d_rows[1];
    dp.cy = d_rows[2];
    dp.cz = d_rows[3];
    dp.pixels = film[0];
    dp.avgs = film[1];
    dp.vars = film[2];
    dp.mean = out[0];
    dp.var = out[1];
    dp.guide = guide;
    dp.weights = weights;
    dp.wsum = wsum;
    dp.unusable = unusable;
    const int rc = denoise_enqueue(nullptr, dp, d, &d->kernel_ms);
    if (rc) return rc;
    if (mean) HIP_TRY(hipMemcpy(mean, out[0], n_pix * S * 8, hipMemcpyDeviceToHost));
    if (var) HIP_TRY(hipMemcpy(var, out[1], n_pix * S * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&d->unusable, unusable, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_denoise_buffers(const drt_scene *scene, const drt_params *params, drt_denoise *d, const double *pixels, const double *avgs,
                                   const double *vars, double *mean, double *var)
{
    g_last_error.clear();
    if (!scene || !params || !d || !pixels || !avgs || !vars) return fail(-1, "null argument");
    int rc = denoise_check(d);
    if (rc) return rc;
    const uint32_t S = scene->num_wavelengths;
    if ((rc = denoise_check_film(params->mode, params->row_stride, S))) return rc;
    if (params->tile_w == 0 || params->tile_h == 0) return fail(-1, "denoise: an empty tile");
    const uint32_t rows[4] = {scene->cmf_rw, scene->cmf_x, scene->cmf_y, scene->cmf_z};
    for (int k = 0; k < 4; k += 1)
        if (rows[k] >= scene->num_spds || !scene->spds) return fail(-1, "denoise: colour-matching row %u of %u SPDs", rows[k], scene->num_spds);
    HIP_TRY(hipSetDevice(params->device));
    DevBuf<double> d_cmf;
    HIP_TRY(d_cmf.need((size_t)4 * S));
    for (int k = 0; k < 4; k += 1)
        HIP_TRY(hipMemcpy(d_cmf + (size_t)k * S, scene->spds + (size_t)rows[k] * S, (size_t)S * 8, hipMemcpyHostToDevice));
    const double *d_rows[4] = {d_cmf, d_cmf + S, d_cmf + 2 * (size_t)S, d_cmf + 3 * (size_t)S};
    return denoise_host_film(d_rows, S, params->tile_w, params->tile_h, scene->wavelength_interval, d, pixels, avgs, vars, mean, var);
}

/* Row-cyclic devices hold no neighbours of their own rows: the group gathers the film (drt_group_read_film) and its first device
 * filters it whole, so the bits are those of one context for any device list. */
extern "C" int drt_group_denoise(drt_group *g, drt_denoise *d, double *mean, double *var)
{
    if (!g || !d) return fail(-1, "null argument");
    int rc = denoise_check(d);
    if (rc) return rc;
    drt_context *first = nullptr;
    for (drt_context *c : g->ctx)
        if (c && !first) first = c;
    if (!first) return fail(-1, "denoise: an empty group");
    /* (a context of a group of n devices has row_stride n x the group's: what counts is the group's own) */
    if ((rc = denoise_check_film(g->xyz_mode ? DRT_MODE_XYZ : DRT_MODE_SPECTRAL, first->params.row_stride / (uint32_t)g->ctx.size(), g->S))) return rc;
    const size_t n_pix = (size_t)g->tile_w * g->tile_h, S = g->S;
    std::vector<double> px(n_pix * (S + 1)), av(n_pix * S), va(n_pix * S);
    if ((rc = drt_group_read_film(g, px.data(), av.data(), va.data()))) return rc;
    HIP_TRY(hipSetDevice(first->device));
    const double *d_rows[4] = {first->dsc.spds + (size_t)first->cmf_rw * S, first->dsc.spds + (size_t)first->cmf_x * S,
                               first->dsc.spds + (size_t)first->cmf_y * S, first->dsc.spds + (size_t)first->cmf_z * S};
    return denoise_host_film(d_rows, g->S, g->tile_w, g->tile_h, first->interval, d, px.data(), av.data(), va.data(), mean, var);
}

/* ---------------------------------------------------------------------------------------------- */
/* First-hit feature buffers (kernels in drt_feature_kernels.h)              */

/* the size rule of stage_surfaces' carve-up (drt_first_hit.h): the scans' rows, the SoA table, the type and material words */
static size_t feature_lds_bytes(uint32_t n_surf)
{
    return (size_t)(SR_STRIDE + SF_COUNT) * n_surf * 8 + (((size_t)2 * n_surf * 4 + 7) & ~(size_t)7);
}

/* one lane per tile pixel, FEATURE_BLOCK to a workgroup */
static dim3 pixel_grid(const drt_context *ctx) { return dim3((uint32_t)((ctx->n_pix + FEATURE_BLOCK - 1) / FEATURE_BLOCK)); }

/* [num_materials][3], the rule's "material colour": sums sequential over ascending wavelength, no contraction (the host is built
 * with -ffp-contract=off, like the kernels) */
static int spectra_read_back(drt_context *ctx);
static int feature_colour_table(const drt_context *ctx, std::vector<double> *table)
{
    const uint32_t S = ctx->ft_S;
    const double *spds = ctx->ft_spds.data();
    const double *rw = spds + (size_t)ctx->cmf_rw * S;
    const double *cmf[3] = {spds + (size_t)ctx->cmf_x * S, spds + (size_t)ctx->cmf_y * S, spds + (size_t)ctx->cmf_z * S};
    double N = 0.0;
    for (uint32_t i = 0; i < S; i += 1) N += (cmf[1][i] * rw[i]);
    N *= ctx->interval;
    const double scale = ctx->interval / N;
    const std::vector<double> zeros(S, 0.0);
    std::vector<double> r(S);
    table->assign(ctx->ft_mats.size() * 3, 0.0);
    for (size_t m = 0; m < ctx->ft_mats.size(); m += 1)
    {
        const drt_material &mat = ctx->ft_mats[m];
        const int32_t idx[4] = {mat.emission_spd, mat.diffuse_spd, mat.glossy_spd, mat.mirror_spd};
        const double *row[4];
        for (int k = 0; k < 4; k += 1)
        {
            if (idx[k] >= 0 && (uint32_t)idx[k] >= ctx->ft_n_spd) return fail(-1, "features: material %zu names SPD %d of %u", m, idx[k], ctx->ft_n_spd);
            row[k] = idx[k] >= 0 ? spds + (size_t)idx[k] * S : zeros.data();
        }
        for (uint32_t i = 0; i < S; i += 1) r[i] = mat.is_emissive ? row[0][i] : (row[1][i] + row[2][i]) + row[3][i];
        for (int k = 0; k < 3; k += 1)
        {
            double acc = 0.0;
            for (uint32_t i = 0; i < S; i += 1) acc += (cmf[k][i] * r[i] * rw[i]);
            (*table)[m * 3 + k] = acc * scale;
        }
    }
    return 0;
}

/* The pixel passes (features, mattes) share what follows; `who` is the pass's name in its messages, "features" or "mattes". */
static int first_hit_check(const char *who, uint32_t flags, uint32_t first_sample, uint32_t n_samples)
{
    if (flags != 0) return fail(-1, "%s: flags = %u: 0 (reserved)", who, flags);
    if (n_samples && (uint64_t)first_sample + n_samples > 0xFFFFFFFFull)
        return fail(-1, "%s: first_sample %u + %u samples: sample numbers are 32 bits", who, first_sample, n_samples);
    return 0;
}

/* n_samples = 0: every tile pixel's count from its filter sum into d_ft_counts, which the feature and the matte pass share (each reads
 * it only in the kernel of the same call). The stream must be idle. */
static int film_counts(drt_context *ctx, const char *who, uint32_t first_sample)
{
    const size_t n_pix = (size_t)ctx->n_pix;
    HIP_TRY(ctx->d_ft_counts.need(n_pix));
    HIP_TRY(ctx->d_ft_report.need(2));
    uint32_t report[2] = {0xFFFFFFFFu, 0u};
    HIP_TRY(hipMemcpyAsync(ctx->d_ft_report, report, sizeof(report), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(drt_feature_counts_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), 0, ctx->stream,
                       ctx->d_pixels, ctx->dsc.S, (uint32_t)n_pix, ctx->d_ft_counts, ctx->d_ft_report);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(report, ctx->d_ft_report, sizeof(report), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (report[0] != 0xFFFFFFFFu)
    {
        double sum = 0.0;
        HIP_TRY(hipMemcpy(&sum, ctx->d_pixels + (size_t)report[0] * (ctx->dsc.S + 1) + ctx->dsc.S, sizeof(sum), hipMemcpyDeviceToHost));
        return fail(-7, "%s: tile pixel %u (column %u, row %u of the tile) holds the filter sum %g: with n_samples = 0 a pixel's sample count is its filter sum, a whole number from 1 to 2^32 - 1 (an empty film has none: give n_samples)",
                    who, report[0], report[0] % ctx->params.tile_w, report[0] / ctx->params.tile_w, sum);
    }
    if ((uint64_t)first_sample + report[1] > 0xFFFFFFFFull)
        return fail(-1, "%s: first_sample %u + %u samples: sample numbers are 32 bits", who, first_sample, report[1]);
    return 0;
}

/* The film complete and the pass's earlier results (*valid) given up. Refuses before anything is rendered; the film, the adaptive
 * counts, the render state and the other pass's buffers stay as they are. The caller allocates its buffers next and then, with
 * n_samples = 0, takes every pixel's count from its filter sum (film_counts). */
static int first_hit_prepare(drt_context *ctx, const char *who, uint32_t n_samples, bool *valid)
{
    if (ctx->rays_bound) return fail(-7, "%s: they are made from the camera's rays, and a ray table is bound (drt_bind_rays with NULL unbinds it)", who);
    if (n_samples == 0 && ctx->xyz_mode)
        return fail(-4, "%s: n_samples = 0 takes every pixel's count from the spectral film's filter column: DRT_MODE_XYZ keeps none (give n_samples)", who);
    if (ctx->n_pix >= 0xFFFFFFFFull) return fail(-1, "%s: a tile of %llu pixels", who, (unsigned long long)ctx->n_pix);
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = drt_synchronize(ctx);
    if (rc) return rc;
    *valid = false;
    return 0;
}

/* what the pixel passes' kernels read of a pass: the tile, the samples, the counts */
static FeatureParams first_hit_params(const drt_context *ctx, uint32_t n_samples, uint32_t first_sample)
{
    const drt_params &p = ctx->params;
    FeatureParams fp{};
    fp.width = p.width; fp.height = p.height; fp.x0 = p.x0; fp.y0 = p.y0;
    fp.tile_w = p.tile_w; fp.tile_h = p.tile_h; fp.row_stride = p.row_stride;
    fp.n_samples = n_samples;
    fp.first_sample = first_sample;
    fp.pixel_scheme = p.pixel_scheme;
    fp.seed = p.seed;
    fp.n_pix = ctx->n_pix;
    fp.counts = n_samples ? nullptr : ctx->d_ft_counts;
    return fp;
}

/* results of a pass (`what`: "feature", "matte") that took its counts from the film are refused once the film has changed */
static int first_hit_current(bool valid, bool from_film, uint64_t gen, uint64_t film_gen, const char *what)
{
    if (!valid) return fail(-4, "no %s buffers: drt_render_%ss first", what, what);
    if (from_film && gen != film_gen)
        return fail(-4, "the film has changed since drt_render_%ss took its counts from it (n_samples = 0): render the %ss again", what, what);
    return 0;
}

static int features_prepare(drt_context *ctx, const drt_features *f)
{
    int rc = first_hit_prepare(ctx, "features", f->n_samples, &ctx->ft_valid);
    if (rc) return rc;
    const size_t n_pix = (size_t)ctx->n_pix;
    HIP_TRY(ctx->d_ft_mean.need(n_pix * DRT_FEATURE_CHANNELS));
    HIP_TRY(ctx->d_ft_m2.need(n_pix * DRT_FEATURE_CHANNELS));
    HIP_TRY(ctx->d_ft_ids.need(n_pix));
    HIP_TRY(ctx->d_ft_info.need(FEATURE_INFO_WORDS));
    HIP_TRY(ctx->d_ft_colour.need(std::max<size_t>(ctx->ft_mats.size(), 1) * 3));
    for (Event &e : ctx->ft_ev) HIP_TRY(e.need());
    return f->n_samples == 0 ? film_counts(ctx, "features", f->first_sample) : 0;
}

static int features_enqueue(drt_context *ctx, const drt_features *f)
{
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<double> table;
    int rc = spectra_read_back(ctx); /* the table is made from the host's mirror of the spectra */
    if (rc) return rc;
    if ((rc = feature_colour_table(ctx, &table))) return rc;
    if (!table.empty()) HIP_TRY(hipMemcpy(ctx->d_ft_colour, table.data(), table.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(ctx->d_ft_info, 0, FEATURE_INFO_WORDS * sizeof(unsigned long long), ctx->stream));
    FeatureParams fp = first_hit_params(ctx, f->n_samples, f->first_sample);
    fp.colour = ctx->d_ft_colour;
    fp.mean = ctx->d_ft_mean;
    fp.m2 = ctx->d_ft_m2;
    fp.ids = ctx->d_ft_ids;
    fp.info = ctx->d_ft_info;
    HIP_TRY(hipEventRecord(ctx->ft_ev[0], ctx->stream));
    if (ctx->scene_in_lds)
        hipLaunchKernelGGL(drt_feature_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), feature_lds_bytes(ctx->dsc.n_surf), ctx->stream, ctx->dsc, ctx->dcam, fp);
    else
        hipLaunchKernelGGL(drt_feature_bvh_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), 0, ctx->stream, ctx->dsc, ctx->dcam, fp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ft_ev[1], ctx->stream));
    return 0;
}

/* waits for the kernel; adds this context's share to the report (kernel_ms: the slowest context's) */
static int features_finish(drt_context *ctx, drt_features *f)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(-100 - (int)e, "feature kernel: %s", hipGetErrorString(e));
    unsigned long long info[FEATURE_INFO_WORDS] = {0, 0};
    HIP_TRY(hipMemcpy(info, ctx->d_ft_info, sizeof(info), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ft_ev[0], ctx->ft_ev[1]));
    f->empty_pixels += (uint32_t)info[0];
    f->rays += info[1];
    f->kernel_ms = std::max(f->kernel_ms, (double)ms);
    ctx->ft_gen = ctx->film_gen;
    ctx->ft_from_film = f->n_samples == 0;
    ctx->ft_valid = true;
    return 0;
}

extern "C" int drt_render_features(drt_context *ctx, drt_features *f)
{
    if (!ctx || !f) return fail(-1, "null argument");
    int rc = first_hit_check("features", f->flags, f->first_sample, f->n_samples);
    if (rc) return rc;
    if ((rc = features_prepare(ctx, f))) return rc;
    if ((rc = features_enqueue(ctx, f))) return rc;
    f->empty_pixels = 0;
    f->rays = 0;
    f->kernel_ms = 0.0;
    return features_finish(ctx, f);
}

static int features_current(drt_context *ctx) { return first_hit_current(ctx->ft_valid, ctx->ft_from_film, ctx->ft_gen, ctx->film_gen, "feature"); }

extern "C" int drt_read_features(drt_context *ctx, double *mean, double *m2, int32_t *ids)
{
    if (!ctx) return fail(-1, "null context");
    int rc = features_current(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->n_pix * DRT_FEATURE_CHANNELS * 8;
    if (mean) HIP_TRY(hipMemcpy(mean, ctx->d_ft_mean, bytes, hipMemcpyDeviceToHost));
    if (m2) HIP_TRY(hipMemcpy(m2, ctx->d_ft_m2, bytes, hipMemcpyDeviceToHost));
    if (ids) HIP_TRY(hipMemcpy(ids, ctx->d_ft_ids, (size_t)ctx->n_pix * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_feature_bgra(drt_context *ctx, int which, double lo, double hi, uint8_t *bgra)
{
    if (!ctx || !bgra) return fail(-1, "null argument");
    if (which < 0 || which > 2) return fail(-1, "features: which = %d: 0 normal, 1 depth, 2 coverage", which);
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) return fail(-1, "features: lo = %g, hi = %g: finite numbers, lo below hi", lo, hi);
    int rc = features_current(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    hipLaunchKernelGGL(drt_feature_bgra_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), 0, ctx->stream,
                       (const double *)ctx->d_ft_mean, ctx->n_pix, which, lo, hi, ctx->d_bgra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

/* every device its own rows, side by side: parameters and films checked on all of them before any renders */
extern "C" int drt_group_render_features(drt_group *g, drt_features *f, double *mean, double *m2, int32_t *ids)
{
    g_last_error.clear();
    if (!g || !f) return fail(-1, "null argument");
    int rc = first_hit_check("features", f->flags, f->first_sample, f->n_samples);
    if (rc) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = features_prepare(c, f))) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = features_enqueue(c, f))) return rc;
    f->empty_pixels = 0;
    f->rays = 0;
    f->kernel_ms = 0.0;
    for (drt_context *c : g->ctx)
        if (c && (rc = features_finish(c, f))) return rc;
    const size_t row8 = (size_t)g->tile_w * DRT_FEATURE_CHANNELS * 8;
    if ((rc = group_gather_rows(g, mean, row8, &drt_context::d_ft_mean))) return rc;
    if ((rc = group_gather_rows(g, m2, row8, &drt_context::d_ft_m2))) return rc;
    return group_gather_rows(g, ids, (size_t)g->tile_w * sizeof(int32_t), &drt_context::d_ft_ids);
}

/* ---------------------------------------------------------------------------------------------- */
/* ID mattes (kernels in drt_matte_kernels.h)                                */

#define MATTE_MAX_IDS 4096u
#define MATTE_WORDS (DRT_MATTE_LAYERS * DRT_MATTE_SLOTS) /* ids and counts per pixel */

static int mattes_prepare(drt_context *ctx, const drt_mattes *m)
{
    int rc = first_hit_prepare(ctx, "mattes", m->n_samples, &ctx->mt_valid);
    if (rc) return rc;
    const size_t n_pix = (size_t)ctx->n_pix;
    HIP_TRY(ctx->d_mt_ids.need(n_pix * MATTE_WORDS));
    HIP_TRY(ctx->d_mt_counts.need(n_pix * MATTE_WORDS));
    HIP_TRY(ctx->d_mt_tail.need(n_pix * 4));
    HIP_TRY(ctx->d_mt_info.need(MATTE_INFO_WORDS));
    for (Event &e : ctx->mt_ev) HIP_TRY(e.need());
    return m->n_samples == 0 ? film_counts(ctx, "mattes", m->first_sample) : 0;
}

static int mattes_enqueue(drt_context *ctx, const drt_mattes *m)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(ctx->d_mt_info, 0, MATTE_INFO_WORDS * sizeof(unsigned long long), ctx->stream));
    MatteParams mp{};
    mp.fp = first_hit_params(ctx, m->n_samples, m->first_sample);
    mp.ids = ctx->d_mt_ids;
    mp.counts = ctx->d_mt_counts;
    mp.tail = ctx->d_mt_tail;
    mp.info = ctx->d_mt_info;
    HIP_TRY(hipEventRecord(ctx->mt_ev[0], ctx->stream));
    if (ctx->scene_in_lds)
        hipLaunchKernelGGL(drt_matte_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), feature_lds_bytes(ctx->dsc.n_surf), ctx->stream, ctx->dsc, ctx->dcam, mp);
    else
        hipLaunchKernelGGL(drt_matte_bvh_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), 0, ctx->stream, ctx->dsc, ctx->dcam, mp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->mt_ev[1], ctx->stream));
    return 0;
}

/* waits for the kernel; adds this context's share to the report (kernel_ms: the slowest context's) */
static int mattes_finish(drt_context *ctx, drt_mattes *m)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(-100 - (int)e, "matte kernel: %s", hipGetErrorString(e));
    unsigned long long info[MATTE_INFO_WORDS] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(info, ctx->d_mt_info, sizeof(info), hipMemcpyDeviceToHost));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->mt_ev[0], ctx->mt_ev[1]));
    m->empty_pixels += (uint32_t)info[0];
    m->overflow_pixels[0] += (uint32_t)info[1];
    m->overflow_pixels[1] += (uint32_t)info[2];
    m->rays += info[3];
    m->kernel_ms = std::max(m->kernel_ms, (double)ms);
    ctx->mt_gen = ctx->film_gen;
    ctx->mt_from_film = m->n_samples == 0;
    ctx->mt_valid = true;
    return 0;
}

static void mattes_clear_out(drt_mattes *m)
{
    m->empty_pixels = 0;
    m->overflow_pixels[0] = m->overflow_pixels[1] = 0;
    m->rays = 0;
    m->kernel_ms = 0.0;
}

extern "C" int drt_render_mattes(drt_context *ctx, drt_mattes *m)
{
    if (!ctx || !m) return fail(-1, "null argument");
    int rc = first_hit_check("mattes", m->flags, m->first_sample, m->n_samples);
    if (rc) return rc;
    if ((rc = mattes_prepare(ctx, m))) return rc;
    if ((rc = mattes_enqueue(ctx, m))) return rc;
    mattes_clear_out(m);
    return mattes_finish(ctx, m);
}

static int mattes_current(drt_context *ctx) { return first_hit_current(ctx->mt_valid, ctx->mt_from_film, ctx->mt_gen, ctx->film_gen, "matte"); }

extern "C" int drt_read_mattes(drt_context *ctx, int32_t *ids, uint32_t *counts, uint32_t *tail)
{
    if (!ctx) return fail(-1, "null context");
    int rc = mattes_current(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n_pix = (size_t)ctx->n_pix;
    if (ids) HIP_TRY(hipMemcpy(ids, ctx->d_mt_ids, n_pix * MATTE_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (counts) HIP_TRY(hipMemcpy(counts, ctx->d_mt_counts, n_pix * MATTE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (tail) HIP_TRY(hipMemcpy(tail, ctx->d_mt_tail, n_pix * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

static int matte_layer_check(int layer)
{
    if (layer != DRT_MATTE_SURFACE && layer != DRT_MATTE_MATERIAL) return fail(-1, "mattes: layer = %d: 0 surfaces, 1 materials", layer);
    return 0;
}

extern "C" int drt_read_matte(drt_context *ctx, int layer, const int32_t *id_list, uint32_t n_ids, double *coverage)
{
    /* what the arguments alone decide comes first, before the context is looked at */
    int rc = matte_layer_check(layer);
    if (rc) return rc;
    if (n_ids == 0 || n_ids > MATTE_MAX_IDS) return fail(-1, "mattes: n_ids = %u: 1 to %u ids", n_ids, MATTE_MAX_IDS);
    if (!id_list || !coverage) return fail(-1, "null argument");
    for (uint32_t k = 0; k < n_ids; k += 1)
        if (id_list[k] < DRT_MATTE_ID_MISS) return fail(-1, "mattes: id_list[%u] = %d: -1 (a miss) or the index of a %s", k, id_list[k], layer == DRT_MATTE_SURFACE ? "surface" : "material");
    if (!ctx) return fail(-1, "null context");
    const uint32_t limit = layer == DRT_MATTE_SURFACE ? ctx->dsc.n_surf : ctx->dsc.n_mat;
    for (uint32_t k = 0; k < n_ids; k += 1)
        if (id_list[k] >= 0 && (uint32_t)id_list[k] >= limit)
            return fail(-1, "mattes: id_list[%u] = %d: the scene has %u %s", k, id_list[k], limit, layer == DRT_MATTE_SURFACE ? "surfaces" : "materials");
    if ((rc = mattes_current(ctx))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->d_mt_list.need(MATTE_MAX_IDS));
    HIP_TRY(ctx->d_mt_cover.need((size_t)ctx->n_pix));
    HIP_TRY(hipMemcpy(ctx->d_mt_list, id_list, n_ids * sizeof(int32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(drt_matte_select_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), 0, ctx->stream,
                       (const int32_t *)ctx->d_mt_ids, (const uint32_t *)ctx->d_mt_counts, (const uint32_t *)ctx->d_mt_tail, ctx->n_pix, layer,
                       (const int32_t *)ctx->d_mt_list, n_ids, ctx->d_mt_cover);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(coverage, ctx->d_mt_cover, (size_t)ctx->n_pix * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_read_matte_bgra(drt_context *ctx, int layer, uint8_t *bgra)
{
    if (!ctx || !bgra) return fail(-1, "null argument");
    int rc = matte_layer_check(layer);
    if (rc) return rc;
    if ((rc = mattes_current(ctx))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->d_bgra.need((size_t)ctx->n_pix * 4));
    hipLaunchKernelGGL(drt_matte_bgra_kernel, pixel_grid(ctx), dim3(FEATURE_BLOCK), 0, ctx->stream,
                       (const int32_t *)ctx->d_mt_ids, (const uint32_t *)ctx->d_mt_counts, (const uint32_t *)ctx->d_mt_tail, ctx->n_pix, layer, ctx->d_bgra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(bgra, ctx->d_bgra, (size_t)ctx->n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

/* every device its own rows, side by side: parameters and films checked on all of them before any renders */
extern "C" int drt_group_render_mattes(drt_group *g, drt_mattes *m, int32_t *ids, uint32_t *counts, uint32_t *tail)
{
    g_last_error.clear();
    if (!g || !m) return fail(-1, "null argument");
    int rc = first_hit_check("mattes", m->flags, m->first_sample, m->n_samples);
    if (rc) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = mattes_prepare(c, m))) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = mattes_enqueue(c, m))) return rc;
    mattes_clear_out(m);
    for (drt_context *c : g->ctx)
        if (c && (rc = mattes_finish(c, m))) return rc;
    const size_t row = (size_t)g->tile_w * MATTE_WORDS * 4;
    if ((rc = group_gather_rows(g, ids, row, &drt_context::d_mt_ids))) return rc;
    if ((rc = group_gather_rows(g, counts, row, &drt_context::d_mt_counts))) return rc;
    return group_gather_rows(g, tail, (size_t)g->tile_w * 4 * 4, &drt_context::d_mt_tail);
}

/* ---------------------------------------------------------------------------------------------- */
/* Ray queries (kernels in drt_ray_kernels.h)                               */

enum { RAYS_CLOSEST = 0, RAYS_VISIBLE = 1, RAYS_PIXELS = 2 };
static const char *const ray_call_name[3] = {"drt_cast_rays", "drt_test_visibility", "drt_cast_pixels"};

/* the caller's arrays of one query list (or of one device's share of it); which of them a call uses depends on its kind */
struct RayArgs
{
    const double *a = nullptr, *b = nullptr; /* origins and dirs, p0 and p1 */
    drt_ray_hit *hits = nullptr;
    uint8_t *visible = nullptr;
    const uint32_t *xy = nullptr, *samples = nullptr;
    double *out_a = nullptr, *out_b = nullptr; /* drt_cast_pixels: the rays cast, either may be null */
};

static RayArgs ray_args_from(const RayArgs &r, uint64_t first)
{
    RayArgs s;
    s.a = r.a ? r.a + first * 3 : nullptr;
    s.b = r.b ? r.b + first * 3 : nullptr;
    s.hits = r.hits ? r.hits + first : nullptr;
    s.visible = r.visible ? r.visible + first : nullptr;
    s.xy = r.xy ? r.xy + first * 2 : nullptr;
    s.samples = r.samples ? r.samples + first : nullptr;
    s.out_a = r.out_a ? r.out_a + first * 3 : nullptr;
    s.out_b = r.out_b ? r.out_b + first * 3 : nullptr;
    return s;
}

/* Everything that can be refused, before any device call. *nothing: the list is empty, a successful no-op. */
static int rays_check(int kind, uint32_t width, uint32_t height, const RayArgs &r, uint64_t n, uint32_t flags, bool *nothing)
{
    const char *who = ray_call_name[kind];
    *nothing = false;
    if (flags & ~DRT_RAYS_DEVICE) return fail(-1, "%s: flags = %u: 0 or DRT_RAYS_DEVICE", who, flags);
    if (n == 0)
    {
        *nothing = true;
        return 0;
    }
    if (kind == RAYS_CLOSEST)
    {
        if (!r.a) return fail(-1, "%s: origins is null", who);
        if (!r.b) return fail(-1, "%s: dirs is null", who);
        if (!r.hits) return fail(-1, "%s: hits is null", who);
    }
    else if (kind == RAYS_VISIBLE)
    {
        if (!r.a) return fail(-1, "%s: p0 is null", who);
        if (!r.b) return fail(-1, "%s: p1 is null", who);
        if (!r.visible) return fail(-1, "%s: visible is null", who);
    }
    else
    {
        if (!r.xy) return fail(-1, "%s: xy is null", who);
        if (!r.samples) return fail(-1, "%s: samples is null", who);
        if (!r.hits) return fail(-1, "%s: hits is null", who);
    }
    if ((flags & DRT_RAYS_DEVICE) && n > (1ull << 31)) return fail(-1, "%s: n = %llu: 2^31 rays at most in device mode", who, (unsigned long long)n);
    if (kind == RAYS_PIXELS && !(flags & DRT_RAYS_DEVICE)) /* (device mode: the host cannot read xy; the kernel gives such a query a NaN ray, a miss) */
        for (uint64_t i = 0; i < n; i += 1)
            if (r.xy[i * 2] >= width || r.xy[i * 2 + 1] >= height)
                return fail(-1, "%s: xy[%llu] = (%u, %u): outside the %u x %u image", who, (unsigned long long)i, r.xy[i * 2], r.xy[i * 2 + 1], width, height);
    return 0;
}

/* one launch over device arrays, on the context's stream */
static int rays_launch(drt_context *ctx, int kind, const RayArgs &d, uint64_t n)
{
    RayParams rp{};
    rp.n = n;
    rp.a = d.a; rp.b = d.b; rp.hits = d.hits; rp.visible = d.visible;
    rp.xy = d.xy; rp.samples = d.samples; rp.out_a = d.out_a; rp.out_b = d.out_b;
    rp.width = ctx->params.width; rp.height = ctx->params.height;
    rp.pixel_scheme = ctx->params.pixel_scheme;
    rp.seed = ctx->params.seed;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + RAY_BLOCK - 1) / RAY_BLOCK, (uint64_t)std::max(1, ctx->ray_grid_cap));
    const size_t lds = feature_lds_bytes(ctx->dsc.n_surf);
    hipStream_t st = ctx->stream;
    if (ctx->scene_in_lds)
    {
        if (kind == RAYS_CLOSEST) hipLaunchKernelGGL(drt_ray_closest_kernel<false>, dim3(grid), dim3(RAY_BLOCK), lds, st, ctx->dsc, ctx->dcam, rp);
        else if (kind == RAYS_PIXELS) hipLaunchKernelGGL(drt_ray_closest_kernel<true>, dim3(grid), dim3(RAY_BLOCK), lds, st, ctx->dsc, ctx->dcam, rp);
        else hipLaunchKernelGGL(drt_ray_visible_kernel, dim3(grid), dim3(RAY_BLOCK), lds, st, ctx->dsc, rp);
    }
    else
    {
        if (kind == RAYS_CLOSEST) hipLaunchKernelGGL(drt_ray_closest_bvh_kernel<false>, dim3(grid), dim3(RAY_BLOCK), 0, st, ctx->dsc, ctx->dcam, rp);
        else if (kind == RAYS_PIXELS) hipLaunchKernelGGL(drt_ray_closest_bvh_kernel<true>, dim3(grid), dim3(RAY_BLOCK), 0, st, ctx->dsc, ctx->dcam, rp);
        else hipLaunchKernelGGL(drt_ray_visible_bvh_kernel, dim3(grid), dim3(RAY_BLOCK), 0, st, ctx->dsc, rp);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Host mode: the list in chunks of ctx->ray_chunk rays through the staging buffers, all on the context's stream and in its order, so
 * a buffer is reused only after the kernel and the copies of the chunk before. Enqueues only; rays_host_finish waits. */
static int rays_host_enqueue(drt_context *ctx, int kind, const RayArgs &h, uint64_t n)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t cap = (size_t)ctx->ray_chunk;
    int rc = 0;
    RayArgs d;
    if (kind != RAYS_PIXELS)
    {
        HIP_TRY(ctx->d_ray_a.need(cap * 3));
        HIP_TRY(ctx->d_ray_b.need(cap * 3));
        d.a = ctx->d_ray_a;
        d.b = ctx->d_ray_b;
    }
    else
    {
        HIP_TRY(ctx->d_ray_xy.need(cap * 2));
        HIP_TRY(ctx->d_ray_samples.need(cap));
        d.xy = ctx->d_ray_xy;
        d.samples = ctx->d_ray_samples;
        if (h.out_a)
        {
            HIP_TRY(ctx->d_ray_a.need(cap * 3));
            d.out_a = ctx->d_ray_a;
        }
        if (h.out_b)
        {
            HIP_TRY(ctx->d_ray_b.need(cap * 3));
            d.out_b = ctx->d_ray_b;
        }
    }
    if (kind == RAYS_VISIBLE)
    {
        HIP_TRY(ctx->d_ray_visible.need(cap));
        d.visible = ctx->d_ray_visible;
    }
    else
    {
        HIP_TRY(ctx->d_ray_hits.need(cap));
        d.hits = ctx->d_ray_hits;
    }
    hipStream_t st = ctx->stream;
    for (uint64_t first = 0; first < n; first += cap)
    {
        const size_t m = (size_t)std::min<uint64_t>(cap, n - first);
        const RayArgs c = ray_args_from(h, first);
        if (kind != RAYS_PIXELS)
        {
            HIP_TRY(hipMemcpyAsync(ctx->d_ray_a, c.a, m * 24, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->d_ray_b, c.b, m * 24, hipMemcpyHostToDevice, st));
        }
        else
        {
            HIP_TRY(hipMemcpyAsync(ctx->d_ray_xy, c.xy, m * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ctx->d_ray_samples, c.samples, m * 4, hipMemcpyHostToDevice, st));
        }
        if ((rc = rays_launch(ctx, kind, d, m))) return rc;
        if (kind == RAYS_VISIBLE) HIP_TRY(hipMemcpyAsync(c.visible, ctx->d_ray_visible, m, hipMemcpyDeviceToHost, st));
        else HIP_TRY(hipMemcpyAsync(c.hits, ctx->d_ray_hits, m * sizeof(drt_ray_hit), hipMemcpyDeviceToHost, st));
        if (kind == RAYS_PIXELS && c.out_a) HIP_TRY(hipMemcpyAsync(c.out_a, ctx->d_ray_a, m * 24, hipMemcpyDeviceToHost, st));
        if (kind == RAYS_PIXELS && c.out_b) HIP_TRY(hipMemcpyAsync(c.out_b, ctx->d_ray_b, m * 24, hipMemcpyDeviceToHost, st));
    }
    return 0;
}

static int rays_host_finish(drt_context *ctx, int kind)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(-100 - (int)e, "%s: %s", ray_call_name[kind], hipGetErrorString(e));
    return 0;
}

static int rays_call(drt_context *ctx, int kind, const RayArgs &r, uint64_t n, uint32_t flags)
{
    g_last_error.clear();
    if (!ctx) return fail(-1, "%s: ctx is null", ray_call_name[kind]);
    if (kind == RAYS_PIXELS && ctx->rays_bound)
        return fail(-7, "%s: it asks for the camera's rays, and a ray table is bound (drt_bind_rays with NULL unbinds it)", ray_call_name[kind]);
    bool nothing = false;
    int rc = rays_check(kind, ctx->params.width, ctx->params.height, r, n, flags, &nothing);
    if (rc || nothing) return rc;
    if (flags & DRT_RAYS_DEVICE)
    {
        HIP_TRY(hipSetDevice(ctx->device));
        return rays_launch(ctx, kind, r, n);
    }
    if ((rc = rays_host_enqueue(ctx, kind, r, n))) return rc;
    return rays_host_finish(ctx, kind);
}

extern "C" int drt_cast_rays(drt_context *ctx, const double *origins, const double *dirs, uint64_t n, drt_ray_hit *hits, uint32_t flags)
{
    RayArgs r;
    r.a = origins; r.b = dirs; r.hits = hits;
    return rays_call(ctx, RAYS_CLOSEST, r, n, flags);
}

extern "C" int drt_test_visibility(drt_context *ctx, const double *p0, const double *p1, uint64_t n, uint8_t *visible, uint32_t flags)
{
    RayArgs r;
    r.a = p0; r.b = p1; r.visible = visible;
    return rays_call(ctx, RAYS_VISIBLE, r, n, flags);
}

extern "C" int drt_cast_pixels(drt_context *ctx, const uint32_t *xy, const uint32_t *samples, uint64_t n, double *origins, double *dirs,
                               drt_ray_hit *hits, uint32_t flags)
{
    RayArgs r;
    r.xy = xy; r.samples = samples; r.out_a = origins; r.out_b = dirs; r.hits = hits;
    return rays_call(ctx, RAYS_PIXELS, r, n, flags);
}

/* The list in contiguous shares, one per device that holds a context, results in list order. Every context holds the same scene, camera,
 * image size and seed, so the bits are one context's. Checked once, before any launch; every device is given its share before any is
 * waited for. */
static int rays_group_call(drt_group *g, int kind, const RayArgs &r, uint64_t n)
{
    g_last_error.clear();
    if (!g) return fail(-1, "%s: the group is null", ray_call_name[kind]);
    std::vector<drt_context *> live;
    for (drt_context *c : g->ctx)
        if (c) live.push_back(c);
    if (live.empty()) return fail(-1, "%s: the group holds no context", ray_call_name[kind]);
    for (drt_context *c : live)
        if (kind == RAYS_PIXELS && c->rays_bound)
            return fail(-7, "%s: it asks for the camera's rays, and a ray table is bound (drt_group_bind_rays with NULL unbinds it)", ray_call_name[kind]);
    bool nothing = false;
    int rc = 0;
    for (drt_context *c : live)
        if ((rc = rays_check(kind, c->params.width, c->params.height, r, n, 0, &nothing)) || nothing) return rc;
    const uint64_t k = live.size();
    for (uint64_t d = 0; d < k; d += 1)
    {
        const uint64_t first = n / k * d + std::min<uint64_t>(d, n % k), count = n / k + (d < n % k ? 1 : 0);
        if (count && (rc = rays_host_enqueue(live[d], kind, ray_args_from(r, first), count))) return rc;
    }
    for (drt_context *c : live)
        if ((rc = rays_host_finish(c, kind))) return rc;
    return 0;
}

extern "C" int drt_group_cast_rays(drt_group *g, const double *origins, const double *dirs, uint64_t n, drt_ray_hit *hits)
{
    RayArgs r;
    r.a = origins; r.b = dirs; r.hits = hits;
    return rays_group_call(g, RAYS_CLOSEST, r, n);
}

extern "C" int drt_group_test_visibility(drt_group *g, const double *p0, const double *p1, uint64_t n, uint8_t *visible)
{
    RayArgs r;
    r.a = p0; r.b = p1; r.visible = visible;
    return rays_group_call(g, RAYS_VISIBLE, r, n);
}

extern "C" int drt_group_cast_pixels(drt_group *g, const uint32_t *xy, const uint32_t *samples, uint64_t n, double *origins, double *dirs, drt_ray_hit *hits)
{
    RayArgs r;
    r.xy = xy; r.samples = samples; r.out_a = origins; r.out_b = dirs; r.hits = hits;
    return rays_group_call(g, RAYS_PIXELS, r, n);
}

/* ---------------------------------------------------------------------------------------------- */
/* Ray films: the first ray from a table (include/drt_hip.h)                           */

/* what makes a call a refusal before anything is touched; t == NULL (unbind) has only the film's state to pass */
static int bind_rays_check(const drt_context *ctx, const drt_ray_table *t, const char *name, bool group)
{
    if (t)
    {
        if (!t->origins || !t->dirs) return fail(-1, "%s: %s is null", name, !t->origins ? "origins" : "dirs");
        if (t->n_layers == 0) return fail(-1, "%s: n_layers is 0 (a table has at least one layer)", name);
        if (t->flags & ~DRT_RAYS_DEVICE) return fail(-1, "%s: unknown flags 0x%x", name, t->flags);
        if (group && (t->flags & DRT_RAYS_DEVICE)) return fail(-1, "%s: host pointers only (DRT_RAYS_DEVICE is per context: drt_bind_rays)", name);
    }
    if (ctx->film_used || ctx->adaptive_done)
        return fail(-7, "%s: the film holds samples, and the first ray cannot change under them: drt_reset_film first", name);
    /* Behind the hierarchy a first direction keeps its length through mirror and glass vertices into drt_bounce_kernel's walk, which
     * is derived for |d| = 1 (drt_kernels.h, RAY_UNIT_TOLERANCE) and which the camera path shares: there is no scan to fall back
     * on, so a table the host can read is looked at here, the tile's rows of every layer. Zero, NaN and infinite directions pass. */
    if (t && !(t->flags & DRT_RAYS_DEVICE) && ctx->use_bvh)
    {
        const drt_params &p = ctx->params;
        for (uint64_t l = 0; l < t->n_layers; l += 1)
            for (uint32_t j = 0; j < p.tile_h; j += 1)
            {
                const uint32_t y = p.y0 + j * p.row_stride;
                const double *row = t->dirs + ((l * p.height + y) * p.width + p.x0) * 3u;
                for (uint32_t i = 0; i < p.tile_w; i += 1)
                {
                    const double *d = row + 3u * i;
                    const bool finite = std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]);
                    const bool zero = d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0;
                    const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
                    if (finite && !zero && !(std::fabs(dd - 1.0) <= RAY_UNIT_TOLERANCE))
                        return fail(-1, "%s: layer %llu, pixel (%u, %u): the direction (%.17g, %.17g, %.17g) is not of unit length (d.d = %.17g, "
                                        "| d.d - 1 | > 2^-42) and the scene is behind the hierarchy, whose walk holds for |d| = 1: normalise the table's directions",
                                    name, (unsigned long long)l, p.x0 + i, y, d[0], d[1], d[2], dd);
                }
            }
    }
    return 0;
}

/* A binding made ready but not yet in force: the table the kernels will read and, in host mode, the device copies behind it. Making it
 * can fail (memory, a copy); putting it in force cannot, so a group makes every context's ready before it changes any. */
struct PendingRays
{
    DevRayTable rt{};
    DevBuf<double> d_new[3]; /* origins, dirs, weights: dropped with the binding unless it is put in force */
    bool        bound = false;
};

static int bind_rays_prepare(drt_context *ctx, const drt_ray_table *t, PendingRays &pr, const char *name)
{
    const drt_params &p = ctx->params;
    HIP_TRY(hipSetDevice(ctx->device));
    pr.bound = t != nullptr;
    if (!t) return 0;
    DevRayTable &rt = pr.rt;
    rt.n_layers = t->n_layers;
    if (t->flags & DRT_RAYS_DEVICE)
    {
        rt.origins = t->origins; rt.dirs = t->dirs; rt.weights = t->weights;
        rt.layer_stride = (uint64_t)p.width * p.height;
        rt.tiled = 0u;
        return 0;
    }
    /* the tile's rows of every layer, packed [n_layers][tile_h][tile_w]: tile pixel (i, j) is image pixel (x0 + i, y0 + j * row_stride) */
    const uint64_t n_tile = ctx->n_pix, entries = n_tile * t->n_layers;
    const double *src[3] = {t->origins, t->dirs, t->weights};
    for (int a = 0; a < 3; a += 1)
    {
        if (!src[a]) continue;
        const size_t per = a < 2 ? 3 : 1;
        const size_t count = (size_t)entries * per;
        double *rows = (double *)malloc(std::max<size_t>(count, 1) * sizeof(double));
        if (!rows) return fail(-3, "%s: out of host memory for %llu table entries", name, (unsigned long long)entries);
        for (uint64_t l = 0; l < t->n_layers; l += 1)
            for (uint32_t j = 0; j < p.tile_h; j += 1)
            {
                const uint64_t from = ((l * p.height + (uint64_t)p.y0 + (uint64_t)j * p.row_stride) * p.width + p.x0) * per;
                memcpy(rows + (l * n_tile + (uint64_t)j * p.tile_w) * per, src[a] + from, (size_t)p.tile_w * per * sizeof(double));
            }
        hipError_t e = pr.d_new[a].need(count);
        if (e == hipSuccess && count) e = hipMemcpy(pr.d_new[a], rows, count * sizeof(double), hipMemcpyHostToDevice);
        free(rows);
        if (e != hipSuccess)
        {
            (void)hipGetLastError();
            return fail(-100 - (int)e, "%s: %s", name, hipGetErrorString(e));
        }
    }
    rt.origins = pr.d_new[0]; rt.dirs = pr.d_new[1]; rt.weights = pr.d_new[2];
    rt.layer_stride = n_tile;
    rt.tiled = 1u;
    return 0;
}

/* cannot fail. No render is in flight (the film holds no samples), so the old copies can go; a query enqueued in device mode does not
 * read them */
static void bind_rays_commit(drt_context *ctx, PendingRays &pr)
{
    (void)hipSetDevice(ctx->device);
    ctx->d_rt_origins = std::move(pr.d_new[0]);
    ctx->d_rt_dirs = std::move(pr.d_new[1]);
    ctx->d_rt_weights = std::move(pr.d_new[2]);
    ctx->rt = pr.rt;
    ctx->rays_bound = pr.bound;
}

extern "C" int drt_bind_rays(drt_context *ctx, const drt_ray_table *t)
{
    g_last_error.clear();
    if (!ctx) return fail(-1, "drt_bind_rays: ctx is null");
    int rc = bind_rays_check(ctx, t, "drt_bind_rays", false);
    if (rc) return rc;
    PendingRays pr;
    if ((rc = bind_rays_prepare(ctx, t, pr, "drt_bind_rays"))) return rc;
    bind_rays_commit(ctx, pr);
    return 0;
}

extern "C" int drt_group_bind_rays(drt_group *g, const drt_ray_table *t)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_bind_rays: the group is null");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = bind_rays_check(c, t, "drt_group_bind_rays", true))) return rc;
    /* every device's copy is made before any context changes: a device that fails leaves the whole group as it was */
    PendingRays pending[64]; /* a group holds 64 devices at most (drt_group_create) */
    const size_t n = g->ctx.size();
    for (size_t k = 0; k < n && !rc; k += 1)
        if (g->ctx[k]) rc = bind_rays_prepare(g->ctx[k], t, pending[k], "drt_group_bind_rays");
    if (rc) return rc; /* the copies made so far go with `pending` */
    for (size_t k = 0; k < n; k += 1)
        if (g->ctx[k]) bind_rays_commit(g->ctx[k], pending[k]);
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* Scene updates: the camera and the surfaces of a live context (include/drt_hip.h)   */

#define DRT_SURFACES_FLAGS (DRT_SURFACES_DEVICE | DRT_SURFACES_REBUILD)

/* the largest |coordinate| of the surfaces' boxes, as BvhBuilder::build takes it */
static double surfaces_extent(const drt_surface *s, size_t n)
{
    double extent = 0.0;
    for (size_t i = 0; i < n; i += 1)
    {
        if (s[i].type != DRT_GEO_SPHERE && s[i].type != DRT_GEO_PLANE) continue;
        double lo[3], hi[3];
        prim_bounds(s[i], lo, hi);
        for (int k = 0; k < 3; k += 1)
        {
            if (std::fabs(lo[k]) < 1e299) extent = std::max(extent, std::fabs(lo[k]));
            if (std::fabs(hi[k]) < 1e299) extent = std::max(extent, std::fabs(hi[k]));
        }
    }
    return extent;
}

/* what the leaf and refit kernels need to know of a tree: where every leaf slot hangs, and the inner nodes level by level */
struct TreeMaps
{
    std::vector<uint32_t> leaf_parent;
    std::vector<uint2>    entries;
    std::vector<uint32_t> level_first;
};

static void tree_maps(const std::vector<BvhNode> &nodes, size_t n_leaf, TreeMaps *m)
{
    m->leaf_parent.assign(std::max<size_t>(n_leaf, 1), 0u);
    std::vector<std::vector<uint2>> level; /* level[d]: the inner nodes d levels below the root */
    std::vector<std::pair<uint32_t, uint32_t>> todo(1, {0u, 0u});
    while (!todo.empty())
    {
        const uint32_t x = todo.back().first, depth = todo.back().second;
        todo.pop_back();
        for (uint32_t c = 0; c < 2; c += 1)
        {
            const BvhNode &nd = nodes[x];
            if (nd.count[c] > 0) m->leaf_parent[(size_t)(-2 - nd.child[c]) >> 3] = x * 2u + c;
            else if (nd.count[c] == 0)
            {
                if (level.size() < depth + 2) level.resize(depth + 2);
                uint2 e;
                e.x = (uint32_t)nd.child[c];
                e.y = x * 2u + c;
                level[depth + 1].push_back(e);
                todo.push_back({(uint32_t)nd.child[c], depth + 1});
            }
        }
    }
    m->entries.clear();
    m->level_first.assign(1, 0u);
    for (size_t d = level.size(); d-- > 1;)
    {
        if (level[d].empty()) continue;
        m->entries.insert(m->entries.end(), level[d].begin(), level[d].end());
        m->level_first.push_back((uint32_t)m->entries.size());
    }
}

/* the maps of ctx->h_nodes to the device (the allocations are sized for any one-surface-per-leaf tree over the same surfaces) */
static int update_upload_maps(drt_context *ctx)
{
    TreeMaps m;
    tree_maps(ctx->h_nodes, ctx->h_order.size(), &m);
    const size_t n_leaf = std::max<size_t>(ctx->h_order.size(), 1);
    HIP_TRY(ctx->d_leaf_parent.need(n_leaf));
    HIP_TRY(ctx->d_levels.need(std::max<size_t>(ctx->h_nodes.size(), 1)));
    HIP_TRY(hipMemcpy(ctx->d_leaf_parent, m.leaf_parent.data(), n_leaf * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!m.entries.empty()) HIP_TRY(hipMemcpy(ctx->d_levels, m.entries.data(), m.entries.size() * sizeof(uint2), hipMemcpyHostToDevice));
    ctx->level_first = m.level_first;
    return 0;
}

/* everything an update needs on the device, made at the first one. Changes nothing a render reads. */
static int update_prepare(drt_context *ctx)
{
    if (ctx->upd_ready) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = ctx->h_surfaces.size();
    if (!ctx->d_raw)
    {
        HIP_TRY(ctx->d_raw.need(n));
        if (n) HIP_TRY(hipMemcpy(ctx->d_raw, ctx->h_surfaces.data(), n * sizeof(drt_surface), hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx->h_stage.need(n));
    if (!ctx->d_light_slot)
    {
        /* the light list is the emissive surfaces in surface order (build_device_scene); types and materials do not change */
        std::vector<int32_t> slot(std::max<size_t>(n, 1), -1);
        int32_t l = 0;
        for (size_t i = 0; i < n; i += 1)
            if (ctx->ft_mats[ctx->h_surfaces[i].material].is_emissive) slot[i] = l++;
        HIP_TRY(ctx->d_light_slot.need(slot.size()));
        HIP_TRY(hipMemcpy(ctx->d_light_slot, slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx->d_upd_status.need(UPD_STATUS_WORDS));
    for (Event &e : ctx->upd_ev) HIP_TRY(e.need());
    if (ctx->use_bvh)
    {
        HIP_TRY(ctx->d_boxes.need(std::max<size_t>(n, 1) * 6));
        int rc = update_upload_maps(ctx);
        if (rc) return rc;
    }
    ctx->upd_ready = true;
    return 0;
}

/* the three kernels, on the context's stream: every table derived again from ALL raw surfaces and the camera's reach */
static int hierarchy_adopt(drt_context *ctx);

/* the derive kernel over all raw surfaces: every column, the boxes and the extent word */
static int update_enqueue_derive(drt_context *ctx)
{
    const uint32_t n = ctx->dsc.n_surf;
    HIP_TRY(hipMemsetAsync(ctx->d_upd_status, 0, UPD_STATUS_WORDS * sizeof(unsigned long long), ctx->stream));
    UpdateTables t;
    t.raw = (const double *)ctx->d_raw.get();
    t.surf = const_cast<double *>(ctx->dsc.surf);
    t.lights = const_cast<double *>(ctx->dsc.lights);
    t.light_slot = ctx->d_light_slot;
    t.boxes = ctx->use_bvh ? ctx->d_boxes : nullptr;
    t.status = ctx->d_upd_status;
    hipLaunchKernelGGL(drt_surface_derive_kernel, dim3((n + UPDATE_BLOCK - 1) / UPDATE_BLOCK), dim3(UPDATE_BLOCK), 0, ctx->stream, ctx->dsc, t);
    HIP_TRY(hipGetLastError());
    ctx->boxes_valid = ctx->use_bvh;
    return 0;
}

static LeafTables update_leaf_tables(drt_context *ctx)
{
    LeafTables lt;
    lt.raw = (const double *)ctx->d_raw.get();
    lt.boxes = ctx->d_boxes;
    lt.leaf_parent = ctx->d_leaf_parent;
    lt.leaf = const_cast<BvhLeafPrim *>(ctx->dsc.bvh_leaf);
    lt.nodes = const_cast<BvhNode *>(ctx->dsc.bvh_nodes);
    lt.status = ctx->d_upd_status;
    return lt;
}

static int update_enqueue(drt_context *ctx)
{
    int rc = hierarchy_adopt(ctx); /* a refit goes level by level, and after a device build only the device knows the levels yet */
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->upd_ev[0], ctx->stream));
    const uint32_t n = ctx->dsc.n_surf;
    if (n > 0)
    {
        if ((rc = update_enqueue_derive(ctx))) return rc;
        const uint32_t n_leaf = (uint32_t)ctx->h_order.size();
        if (ctx->use_bvh && n_leaf > 0)
        {
            const LeafTables lt = update_leaf_tables(ctx);
            hipLaunchKernelGGL(drt_bvh_leaf_kernel, dim3((n_leaf + UPDATE_BLOCK - 1) / UPDATE_BLOCK), dim3(UPDATE_BLOCK), 0, ctx->stream, lt, n_leaf, ctx->cam_reach);
            HIP_TRY(hipGetLastError());
            for (size_t l = 0; l + 1 < ctx->level_first.size(); l += 1) /* deepest level first; a kernel boundary between two levels */
            {
                const uint32_t first = ctx->level_first[l], cnt = ctx->level_first[l + 1] - first;
                hipLaunchKernelGGL(drt_bvh_refit_kernel, dim3((cnt + UPDATE_BLOCK - 1) / UPDATE_BLOCK), dim3(UPDATE_BLOCK), 0, ctx->stream, lt.nodes, ctx->d_levels + first, cnt);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    HIP_TRY(hipEventRecord(ctx->upd_ev[1], ctx->stream));
    ctx->upd_timed = true;
    ctx->updates += 1;
    if (ctx->use_bvh) ctx->refits += 1;
    /* what describes the old scene is stale */
    ctx->ft_valid = ctx->mt_valid = false;
    return 0;
}

static int update_film_check(const drt_context *ctx, const char *name)
{
    if (ctx->film_used || ctx->adaptive_done)
        return fail(-7, "%s: the film holds samples, and one film would mix two scenes: drt_reset_film first", name);
    return 0;
}

/* a host-mode update that has passed every check, and (DRT_SURFACES_REBUILD) the tree it will install */
struct PendingUpdate
{
    BvhBuilder bb;
    bool       rebuild = false;
    double     extent = 0.0;
};

/* the host copy again after device-mode updates (type and material words are the host's own: device mode does not copy them) */
static int update_read_back(drt_context *ctx)
{
    if (!ctx->h_stale) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!ctx->h_surfaces.empty())
        HIP_TRY(hipMemcpy(ctx->h_surfaces.data(), ctx->d_raw, ctx->h_surfaces.size() * sizeof(drt_surface), hipMemcpyDeviceToHost));
    ctx->h_stale = false;
    ctx->win_dirty = true; /* the host knows the bounds again */
    return 0;
}

/* everything a host-mode call can be refused for; changes nothing */
static int update_check(drt_context *ctx, const drt_surface *surfaces, uint32_t first, uint32_t count, uint32_t flags, const char *name, bool group,
                        PendingUpdate *pu)
{
    const size_t n = ctx->h_surfaces.size();
    if (flags & ~DRT_SURFACES_FLAGS) return fail(-1, "%s: unknown flags 0x%x", name, flags);
    if ((flags & DRT_SURFACES_DEVICE) && (flags & DRT_SURFACES_REBUILD))
        return fail(-1, "%s: DRT_SURFACES_REBUILD builds the hierarchy on the host and needs host surfaces", name);
    if (group && (flags & DRT_SURFACES_DEVICE)) return fail(-1, "%s: host pointers only (DRT_SURFACES_DEVICE is per context: drt_update_surfaces)", name);
    if ((uint64_t)first + count > n) return fail(-1, "%s: surfaces [%u, %llu) of %zu", name, first, (unsigned long long)first + count, n);
    if (count > 0 && !surfaces) return fail(-1, "%s: surfaces is null", name);
    if (count == 0) return 0; /* a no-op, whatever the film holds */
    int rc = update_film_check(ctx, name);
    if (rc) return rc;
    if (flags & DRT_SURFACES_DEVICE) return 0;
    if ((rc = update_read_back(ctx))) return rc;
    for (uint32_t i = 0; i < count; i += 1)
    {
        const drt_surface &was = ctx->h_surfaces[first + i];
        if (surfaces[i].type != was.type) return fail(-2, "%s: surface %u: type %u, was %u (an update keeps every surface's type)", name, first + i, surfaces[i].type, was.type);
        if (surfaces[i].material != was.material)
            return fail(-2, "%s: surface %u: material %u, was %u (an update keeps every surface's material)", name, first + i, surfaces[i].material, was.material);
    }
    if (!ctx->use_bvh) return 0;
    std::vector<drt_surface> all = ctx->h_surfaces;
    std::copy(surfaces, surfaces + count, all.begin() + first);
    pu->rebuild = (flags & DRT_SURFACES_REBUILD) != 0u;
    if (pu->rebuild)
    {
        drt_scene sc{};
        sc.num_surfaces = (uint32_t)n;
        sc.surfaces = all.data();
        pu->bb.build(&sc, ctx->cam_reach);
        pu->extent = pu->bb.extent;
        if (pu->bb.max_depth > BVH_STACK)
            return fail(-2, "%s: BVH of %zu surfaces is %d levels deep, the traversal stack holds %d", name, pu->bb.prims.size(), pu->bb.max_depth, BVH_STACK);
        if (pu->bb.nodes.size() != ctx->h_nodes.size() || pu->bb.order.size() != ctx->h_order.size())
            return fail(-2, "%s: the rebuilt hierarchy has %zu nodes, the context's %zu", name, pu->bb.nodes.size(), ctx->h_nodes.size());
    }
    else pu->extent = std::max(ctx->cam_reach, surfaces_extent(all.data(), n));
    if (!(pu->extent < UPDATE_EXTENT_LIMIT))
        return fail(-2, "%s: scene or camera coordinates reach %g: the hierarchy's f32 box test holds up to 2^27", name, pu->extent);
    return 0;
}

/* the caller's records into the pinned buffer: can fail, and changes nothing a render reads */
static int update_stage(drt_context *ctx, const drt_surface *surfaces, uint32_t count)
{
    int rc = update_prepare(ctx);
    if (rc) return rc;
    if (ctx->stage_busy) HIP_TRY(hipEventSynchronize(ctx->upd_ev[2])); /* the last update's copy out of it */
    ctx->stage_busy = false;
    memcpy(ctx->h_stage, surfaces, (size_t)count * sizeof(drt_surface));
    return 0;
}

static int update_commit(drt_context *ctx, uint32_t first, uint32_t count, PendingUpdate *pu)
{
    HIP_TRY(hipSetDevice(ctx->device));
    std::copy(ctx->h_stage.get(), ctx->h_stage + count, ctx->h_surfaces.begin() + first);
    ctx->win_dirty = true;
    HIP_TRY(hipMemcpyAsync(ctx->d_raw + first, ctx->h_stage, (size_t)count * sizeof(drt_surface), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->upd_ev[2], ctx->stream));
    ctx->stage_busy = true;
    if (pu->rebuild)
    {
        /* nodes and leaf order into the same allocations; the kernels below fill in every box and every leaf's numbers */
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->hb_mirror_pending = false; /* (a device-built tree's links on their way back: this tree replaces them) */
        ctx->hb_built_by = 0;
        ctx->hb_depth = (uint32_t)pu->bb.max_depth;
        std::vector<BvhLeafPrim> leaf(std::max<size_t>(pu->bb.order.size(), 1));
        memset(leaf.data(), 0, leaf.size() * sizeof(BvhLeafPrim));
        for (size_t k = 0; k < pu->bb.order.size(); k += 1)
        {
            leaf[k].index = pu->bb.order[k];
            leaf[k].type = ctx->h_surfaces[pu->bb.order[k]].type;
            leaf[k].reach32 = INFINITY;
        }
        HIP_TRY(hipMemcpy(const_cast<BvhNode *>(ctx->dsc.bvh_nodes), pu->bb.nodes.data(), pu->bb.nodes.size() * sizeof(BvhNode), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(const_cast<BvhLeafPrim *>(ctx->dsc.bvh_leaf), leaf.data(), leaf.size() * sizeof(BvhLeafPrim), hipMemcpyHostToDevice));
        ctx->h_nodes = pu->bb.nodes;
        ctx->h_order = pu->bb.order;
        int rc = update_upload_maps(ctx);
        if (rc) return rc;
    }
    int rc = update_enqueue(ctx);
    if (rc) return rc;
    if (pu->rebuild) ctx->refits = 0;
    ctx->extent = pu->extent;
    ctx->extent_known = true;
    ctx->upd_check = ctx->upd_violation = false; /* the host has checked the extent itself */
    return 0;
}

extern "C" int drt_update_surfaces(drt_context *ctx, const drt_surface *surfaces, uint32_t first, uint32_t count, uint32_t flags)
{
    g_last_error.clear();
    if (!ctx) return fail(-1, "drt_update_surfaces: ctx is null");
    PendingUpdate pu;
    int rc = update_check(ctx, surfaces, first, count, flags, "drt_update_surfaces", false, &pu);
    if (rc || count == 0) return rc;
    if (flags & DRT_SURFACES_DEVICE)
    {
        if ((rc = update_prepare(ctx))) return rc;
        /* the 13 doubles behind the type and material words, record by record, in stream order */
        HIP_TRY(hipMemcpy2DAsync((char *)(ctx->d_raw + first) + 8, sizeof(drt_surface), (const char *)surfaces + 8, sizeof(drt_surface), sizeof(drt_surface) - 8, count,
                                 hipMemcpyDeviceToDevice, ctx->stream));
        ctx->h_stale = true;
        ctx->win_dirty = true; /* the host cannot know the bounds: the live window is the whole tile until it does */
        if ((rc = update_enqueue(ctx))) return rc;
        ctx->extent_known = !ctx->use_bvh;
        ctx->upd_check = ctx->use_bvh;
        ctx->upd_violation = false;
        return 0;
    }
    if ((rc = update_stage(ctx, surfaces, count))) return rc;
    return update_commit(ctx, first, count, &pu);
}

static int set_camera_check(drt_context *ctx, const drt_camera *camera, const char *name)
{
    if (!camera) return fail(-1, "%s: camera is null", name);
    int rc = update_film_check(ctx, name);
    if (rc) return rc;
    const double reach = camera_reach(camera);
    if (ctx->use_bvh && !(reach < UPDATE_EXTENT_LIMIT))
        return fail(-2, "%s: scene or camera coordinates reach %g: the hierarchy's f32 box test holds up to 2^27", name, reach);
    return 0;
}

static int set_camera_commit(drt_context *ctx, const drt_camera *camera)
{
    set_device_camera(ctx, camera); /* kernels take it by value: what is enqueued already keeps the old one */
    ctx->cam_reach = camera_reach(camera);
    if (!ctx->use_bvh)
    {
        ctx->updates += 1;
        ctx->upd_timed = false;
        ctx->upd_ms = 0.0;
        ctx->ft_valid = ctx->mt_valid = false;
        return 0;
    }
    /* the camera's reach is part of the extent, and the extent is in every leaf's padding */
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = update_enqueue(ctx);
    if (rc) return rc;
    ctx->extent_known = false;
    ctx->upd_check = ctx->h_stale; /* the host's own surfaces were checked when they came */
    ctx->upd_violation = false;
    return 0;
}

extern "C" int drt_set_camera(drt_context *ctx, const drt_camera *camera)
{
    g_last_error.clear();
    if (!ctx) return fail(-1, "drt_set_camera: ctx is null");
    int rc = set_camera_check(ctx, camera, "drt_set_camera");
    if (rc) return rc;
    if (ctx->use_bvh && (rc = update_prepare(ctx))) return rc;
    return set_camera_commit(ctx, camera);
}

extern "C" int drt_get_update_report(drt_context *ctx, drt_update_report *out)
{
    g_last_error.clear();
    if (!ctx || !out) return fail(-1, "drt_get_update_report: null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->upd_timed)
    {
        float ms = 0.0f;
        HIP_TRY(hipEventSynchronize(ctx->upd_ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, ctx->upd_ev[0], ctx->upd_ev[1]));
        ctx->upd_ms = (double)ms;
        ctx->upd_timed = false;
    }
    if (ctx->use_bvh && !ctx->extent_known)
    {
        unsigned long long bits = 0;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(&bits, ctx->d_upd_status, sizeof(bits), hipMemcpyDeviceToHost));
        double surfaces = 0.0;
        memcpy(&surfaces, &bits, sizeof(surfaces));
        ctx->extent = std::max(ctx->cam_reach, surfaces);
        ctx->extent_known = true;
    }
    out->updates = ctx->updates;
    out->refits_since_build = ctx->refits;
    out->extent = ctx->use_bvh ? ctx->extent : 0.0;
    out->kernel_ms = ctx->upd_ms;
    return 0;
}

extern "C" int drt_group_set_camera(drt_group *g, const drt_camera *camera)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_set_camera: the group is null");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = set_camera_check(c, camera, "drt_group_set_camera"))) return rc;
    for (drt_context *c : g->ctx)
        if (c && c->use_bvh && (rc = update_prepare(c))) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = set_camera_commit(c, camera))) return rc;
    return 0;
}

extern "C" int drt_group_update_surfaces(drt_group *g, const drt_surface *surfaces, uint32_t first, uint32_t count, uint32_t flags)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_update_surfaces: the group is null");
    int rc = 0;
    /* every context is checked, and every device's staging copy is made, before any context changes */
    std::vector<PendingUpdate> pending(g->ctx.size());
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = update_check(g->ctx[k], surfaces, first, count, flags, "drt_group_update_surfaces", true, &pending[k]))) return rc;
    if (count == 0) return 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = update_stage(c, surfaces, count))) return rc;
    for (size_t k = 0; k < g->ctx.size(); k += 1)
        if (g->ctx[k] && (rc = update_commit(g->ctx[k], first, count, &pending[k]))) return rc;
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* Material updates: new spectra and parameters for a live context (include/drt_hip.h) */

/* everything a material update needs on the device, made at the first one. Changes nothing a render reads. */
static int material_prepare(drt_context *ctx)
{
    if (ctx->mu_ready) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n_mat = ctx->ft_mats.size();
    const size_t row_words = (size_t)ctx->ft_n_spd * ctx->ft_S;
    if (!ctx->d_spd_raw)
    {
        /* the raw copy starts as the mirror, so the mirror must be the device's: this is the first update, and it is */
        HIP_TRY(ctx->d_spd_raw.need(row_words));
        if (!ctx->ft_spds.empty()) HIP_TRY(hipMemcpy(ctx->d_spd_raw, ctx->ft_spds.data(), ctx->ft_spds.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx->d_spd_in.need(row_words));
    HIP_TRY(ctx->h_spd_stage.need(row_words));
    HIP_TRY(ctx->h_mat_stage.need(n_mat));
    if (!ctx->d_spd_desc)
    {
        HIP_TRY(ctx->d_spd_desc.need(ctx->spd_desc.size()));
        if (!ctx->spd_desc.empty())
            HIP_TRY(hipMemcpy(ctx->d_spd_desc, ctx->spd_desc.data(), ctx->spd_desc.size() * sizeof(SpdRowDesc), hipMemcpyHostToDevice));
    }
    if (!ctx->d_mat_refract)
    {
        /* a given refract spectrum is a scene row, and scene rows keep their numbers in the device table */
        std::vector<int32_t> refract(std::max<size_t>(n_mat, 1), -1);
        for (size_t m = 0; m < n_mat; m += 1) refract[m] = ctx->ft_mats[m].refract_spd >= 0 ? ctx->ft_mats[m].refract_spd : -1;
        HIP_TRY(ctx->d_mat_refract.need(refract.size()));
        HIP_TRY(hipMemcpy(ctx->d_mat_refract, refract.data(), refract.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    for (Event &e : ctx->mu_ev) HIP_TRY(e.need());
    ctx->mu_ready = true;
    return 0;
}

/* host_mats' two samples around trans_wl from the mirror, as build_device_scene takes them */
static void material_refract_samples(drt_context *ctx)
{
    const uint32_t S = ctx->ft_S;
    for (size_t m = 0; m < ctx->ft_mats.size(); m += 1)
    {
        const int32_t r = ctx->ft_mats[m].refract_spd;
        if (r < 0) continue;
        ctx->host_mats[m].refract_i0 = ctx->ft_spds[(size_t)r * S + ctx->dsc.trans_i0];
        ctx->host_mats[m].refract_i1 = ctx->ft_spds[(size_t)r * S + ctx->dsc.trans_i0 + 1];
    }
    ctx->variants_stale = true;
}

/* the host mirrors again after device-mode updates (update_read_back's twin): ft_spds from the raw copy, and from it host_mats' refract samples */
static int spectra_read_back(drt_context *ctx)
{
    if (!ctx->spd_stale) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!ctx->ft_spds.empty()) HIP_TRY(hipMemcpy(ctx->ft_spds.data(), ctx->d_spd_raw, ctx->ft_spds.size() * sizeof(double), hipMemcpyDeviceToHost));
    material_refract_samples(ctx);
    ctx->spd_stale = false;
    return 0;
}

/* everything drt_update_spectra can be refused for; changes nothing */
static int spectra_check(drt_context *ctx, const double *rows, uint32_t first_row, uint32_t count, uint32_t flags, const char *name, bool group)
{
    if (flags & ~DRT_SPECTRA_DEVICE) return fail(-1, "%s: unknown flags 0x%x", name, flags);
    if (group && (flags & DRT_SPECTRA_DEVICE)) return fail(-1, "%s: host pointers only (DRT_SPECTRA_DEVICE is per context: drt_update_spectra)", name);
    if ((uint64_t)first_row + count > ctx->ft_n_spd)
        return fail(-1, "%s: rows [%u, %llu) of %u", name, first_row, (unsigned long long)first_row + count, ctx->ft_n_spd);
    if (count > 0 && !rows) return fail(-1, "%s: rows is null", name);
    if (count == 0) return 0; /* a no-op, whatever the film holds */
    const uint32_t cmf[4] = {ctx->cmf_rw, ctx->cmf_x, ctx->cmf_y, ctx->cmf_z};
    static const char *const cmf_name[4] = {"cmf_rw", "cmf_x", "cmf_y", "cmf_z"};
    for (int k = 0; k < 4; k += 1)
        if (cmf[k] >= first_row && cmf[k] - first_row < count)
            return fail(-2, "%s: row %u is the scene's %s (the observer's rows are no material: an update keeps them)", name, cmf[k], cmf_name[k]);
    return update_film_check(ctx, name);
}

/* the caller's rows into the pinned buffer: can fail, and changes nothing a render reads */
static int spectra_stage(drt_context *ctx, const double *rows, uint32_t count)
{
    int rc = material_prepare(ctx);
    if (rc) return rc;
    if ((rc = spectra_read_back(ctx))) return rc;
    if (ctx->spd_stage_busy) HIP_TRY(hipEventSynchronize(ctx->mu_ev[0])); /* the last update's copy out of it */
    ctx->spd_stage_busy = false;
    memcpy(ctx->h_spd_stage, rows, (size_t)count * ctx->ft_S * sizeof(double));
    return 0;
}

/* the two kernels, on the context's stream: every derived row, the refract samples and the tail columns again from ALL raw rows */
static int spectra_enqueue(drt_context *ctx, const double *d_rows, uint32_t first_row, uint32_t count)
{
    const DevScene &d = ctx->dsc;
    SpectraTables t;
    t.src = d_rows;
    t.raw = ctx->d_spd_raw;
    t.table = const_cast<double *>(d.spds);
    t.desc = ctx->d_spd_desc;
    t.first_row = first_row; t.count = count; t.n_spd = d.n_spd; t.S = d.S;
    const uint64_t lanes = (uint64_t)d.n_spd * d.S;
    hipLaunchKernelGGL(drt_spectra_derive_kernel, dim3((uint32_t)((lanes + MATERIAL_BLOCK - 1) / MATERIAL_BLOCK)), dim3(MATERIAL_BLOCK), 0, ctx->stream, t);
    HIP_TRY(hipGetLastError());
    SpectraFinish f;
    f.table = d.spds;
    f.mats = const_cast<DevMaterial *>(d.mats);
    f.mat_refract = ctx->d_mat_refract;
    f.tail = ctx->trace_tail ? const_cast<double *>(ctx->d_spd_tail) : nullptr;
    f.n_mat = d.n_mat; f.n_spd = d.n_spd; f.S = d.S; f.trans_i0 = d.trans_i0;
    f.tail_first = ctx->tail_first; f.tail_count = ctx->tail_count;
    const uint64_t lanes2 = (uint64_t)d.n_mat + (f.tail ? (uint64_t)d.n_spd * ctx->tail_count : 0);
    hipLaunchKernelGGL(drt_spectra_finish_kernel, dim3((uint32_t)((lanes2 + MATERIAL_BLOCK - 1) / MATERIAL_BLOCK)), dim3(MATERIAL_BLOCK), 0, ctx->stream, f);
    HIP_TRY(hipGetLastError());
    ctx->spectra_updates += 1;
    ctx->ft_valid = ctx->mt_valid = false; /* what describes the old scene is stale */
    return 0;
}

static int spectra_commit(drt_context *ctx, uint32_t first_row, uint32_t count)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t words = (size_t)count * ctx->ft_S;
    std::copy(ctx->h_spd_stage.get(), ctx->h_spd_stage + words, ctx->ft_spds.begin() + (size_t)first_row * ctx->ft_S);
    material_refract_samples(ctx);
    HIP_TRY(hipMemcpyAsync(ctx->d_spd_in, ctx->h_spd_stage, words * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->mu_ev[0], ctx->stream));
    ctx->spd_stage_busy = true;
    return spectra_enqueue(ctx, ctx->d_spd_in, first_row, count);
}

extern "C" int drt_update_spectra(drt_context *ctx, const double *rows, uint32_t first_row, uint32_t count, uint32_t flags)
{
    g_last_error.clear();
    if (!ctx) return fail(-1, "drt_update_spectra: ctx is null");
    int rc = spectra_check(ctx, rows, first_row, count, flags, "drt_update_spectra", false);
    if (rc || count == 0) return rc;
    if (flags & DRT_SPECTRA_DEVICE)
    {
        if ((rc = material_prepare(ctx))) return rc;
        HIP_TRY(hipSetDevice(ctx->device));
        ctx->spd_stale = true;
        ctx->variants_stale = true;
        return spectra_enqueue(ctx, rows, first_row, count);
    }
    if ((rc = spectra_stage(ctx, rows, count))) return rc;
    return spectra_commit(ctx, first_row, count);
}

extern "C" int drt_group_update_spectra(drt_group *g, const double *rows, uint32_t first_row, uint32_t count, uint32_t flags)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_update_spectra: the group is null");
    int rc = 0;
    /* every context is checked, and every device's staging copy is made, before any context changes */
    for (drt_context *c : g->ctx)
        if (c && (rc = spectra_check(c, rows, first_row, count, flags, "drt_group_update_spectra", true))) return rc;
    if (count == 0) return 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = spectra_stage(c, rows, count))) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = spectra_commit(c, first_row, count))) return rc;
    return 0;
}

/* everything drt_update_materials can be refused for; changes nothing */
static int materials_check(drt_context *ctx, const drt_material *materials, uint32_t first, uint32_t count, uint32_t flags, const char *name)
{
    const size_t n = ctx->ft_mats.size();
    if (flags != 0) return fail(-1, "%s: unknown flags 0x%x", name, flags);
    if ((uint64_t)first + count > n) return fail(-1, "%s: materials [%u, %llu) of %zu", name, first, (unsigned long long)first + count, n);
    if (count > 0 && !materials) return fail(-1, "%s: materials is null", name);
    if (count == 0) return 0; /* a no-op, whatever the film holds */
    int rc = update_film_check(ctx, name);
    if (rc) return rc;
    for (uint32_t i = 0; i < count; i += 1)
    {
        const drt_material &is = materials[i], &was = ctx->ft_mats[first + i];
        const uint32_t m = first + i;
#define DRT_MATERIAL_KEEPS(field, fmt)                                                                                                     \
    if (is.field != was.field)                                                                                                             \
        return fail(-2, "%s: material %u: " #field " " fmt ", was " fmt " (an update changes shininess and roughness only)", name, m, is.field, was.field)
        DRT_MATERIAL_KEEPS(is_black_body, "%u");
        DRT_MATERIAL_KEEPS(is_emissive, "%u");
        DRT_MATERIAL_KEEPS(emission_spd, "%d");
        DRT_MATERIAL_KEEPS(diffuse_spd, "%d");
        DRT_MATERIAL_KEEPS(glossy_spd, "%d");
        DRT_MATERIAL_KEEPS(mirror_spd, "%d");
        DRT_MATERIAL_KEEPS(refract_spd, "%d");
        DRT_MATERIAL_KEEPS(extinct_spd, "%d");
        DRT_MATERIAL_KEEPS(num_bdsfs, "%u");
        for (uint32_t j = 0; j < std::min<uint32_t>(was.num_bdsfs, DRT_MAX_BDSFS); j += 1)
            if (is.bdsfs[j] != was.bdsfs[j])
                return fail(-2, "%s: material %u: bdsfs[%u] %u, was %u (an update changes shininess and roughness only)", name, m, j, is.bdsfs[j], was.bdsfs[j]);
        DRT_MATERIAL_KEEPS(dir_func, "%u");
#undef DRT_MATERIAL_KEEPS
    }
    return 0;
}

/* the records as the device will hold them, into the pinned buffer: can fail, and changes nothing a render reads */
static int materials_stage(drt_context *ctx, const drt_material *materials, uint32_t first, uint32_t count)
{
    int rc = material_prepare(ctx);
    if (rc) return rc;
    if ((rc = spectra_read_back(ctx))) return rc; /* the records carry refract_i0 / refract_i1 */
    if (ctx->mat_stage_busy) HIP_TRY(hipEventSynchronize(ctx->mu_ev[1]));
    ctx->mat_stage_busy = false;
    for (uint32_t i = 0; i < count; i += 1)
    {
        DevMaterial dm = ctx->host_mats[first + i];
        dm.shininess = materials[i].shininess;
        dm.roughness = materials[i].roughness;
        ctx->h_mat_stage[i] = dm;
    }
    return 0;
}

static int materials_commit(drt_context *ctx, uint32_t first, uint32_t count)
{
    HIP_TRY(hipSetDevice(ctx->device));
    for (uint32_t i = 0; i < count; i += 1)
    {
        ctx->host_mats[first + i] = ctx->h_mat_stage[i];
        ctx->ft_mats[first + i].shininess = ctx->h_mat_stage[i].shininess;
        ctx->ft_mats[first + i].roughness = ctx->h_mat_stage[i].roughness;
    }
    ctx->variants_stale = true;
    HIP_TRY(hipMemcpyAsync(const_cast<DevMaterial *>(ctx->dsc.mats) + first, ctx->h_mat_stage, (size_t)count * sizeof(DevMaterial), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->mu_ev[1], ctx->stream));
    ctx->mat_stage_busy = true;
    ctx->material_updates += 1;
    ctx->ft_valid = ctx->mt_valid = false;
    return 0;
}

extern "C" int drt_update_materials(drt_context *ctx, const drt_material *materials, uint32_t first, uint32_t count, uint32_t flags)
{
    g_last_error.clear();
    if (!ctx) return fail(-1, "drt_update_materials: ctx is null");
    int rc = materials_check(ctx, materials, first, count, flags, "drt_update_materials");
    if (rc || count == 0) return rc;
    if ((rc = materials_stage(ctx, materials, first, count))) return rc;
    return materials_commit(ctx, first, count);
}

extern "C" int drt_group_update_materials(drt_group *g, const drt_material *materials, uint32_t first, uint32_t count, uint32_t flags)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_update_materials: the group is null");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = materials_check(c, materials, first, count, flags, "drt_group_update_materials"))) return rc;
    if (count == 0) return 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = materials_stage(c, materials, first, count))) return rc;
    for (drt_context *c : g->ctx)
        if (c && (rc = materials_commit(c, first, count))) return rc;
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* Device hierarchy builds: the tree of a live context anew, on its stream (include/drt_hip.h) */

/* hb_mirror: the nodes, the surface of every leaf slot, the level counts */
static size_t hierarchy_mirror_order(const drt_context *ctx) { return ctx->h_nodes.size() * sizeof(BvhNode); }
static size_t hierarchy_mirror_counts(const drt_context *ctx) { return hierarchy_mirror_order(ctx) + ctx->h_order.size() * sizeof(uint32_t); }

/* the deepest level an inner node can be on: the rule's budget keeps depth + 2 + ceil(log2 range) <= BVH_STACK, and a chain of
 * inner nodes that deep takes as many surfaces */
static uint32_t hierarchy_max_level(uint32_t m) { return std::min<uint32_t>(BUILD_LEVELS - 2, m - 2u); }

/* the temporaries of a build, made at the first one (with everything an update needs: the raw surfaces, the boxes, the maps) */
static int hierarchy_prepare(drt_context *ctx)
{
    int rc = update_prepare(ctx);
    if (rc || ctx->hb_ready) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t m = ctx->h_order.size(), m1 = std::max<size_t>(m, 1);
    if (!ctx->d_hb_tree_surf)
    {
        std::vector<uint32_t> tree_surf; /* spheres and planes in surface order: types do not change */
        for (size_t i = 0; i < ctx->h_surfaces.size(); i += 1)
            if (ctx->h_surfaces[i].type == DRT_GEO_SPHERE || ctx->h_surfaces[i].type == DRT_GEO_PLANE) tree_surf.push_back((uint32_t)i);
        if (tree_surf.size() != m) return fail(-2, "drt_rebuild_hierarchy: %zu surfaces for a tree of %zu leaf slots", tree_surf.size(), m);
        HIP_TRY(ctx->d_hb_tree_surf.need(m1));
        if (m) HIP_TRY(hipMemcpy(ctx->d_hb_tree_surf, tree_surf.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    const size_t n_tiles = (m1 + SORT_TILE - 1) / SORT_TILE;
    for (int k = 0; k < 2; k += 1)
    {
        HIP_TRY(ctx->d_hb_keys[k].need(m1));
        HIP_TRY(ctx->d_hb_pos[k].need(m1));
        HIP_TRY(ctx->d_hb_items[k].need(m1 / 2 + 1)); /* an item covers two surfaces at least */
    }
    HIP_TRY(ctx->d_hb_table.need((size_t)SORT_DIGITS * n_tiles));
    HIP_TRY(ctx->d_hb_order.need(m1));
    HIP_TRY(ctx->d_hb_status.need(BUILD_STATUS_BYTES));
    HIP_TRY(ctx->hb_mirror.need(hierarchy_mirror_counts(ctx) + (BUILD_LEVELS + 1) * sizeof(uint32_t)));
    for (Event &e : ctx->hb_ev) HIP_TRY(e.need());
    ctx->hb_ready = true;
    return 0;
}

/* the host's copy of a device-built tree, when something needs it: waits for the copy the build enqueued, never for more */
static int hierarchy_adopt(drt_context *ctx)
{
    if (!ctx->hb_mirror_pending) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(ctx->hb_ev[2]));
    memcpy(ctx->h_nodes.data(), ctx->hb_mirror, hierarchy_mirror_order(ctx));
    memcpy(ctx->h_order.data(), ctx->hb_mirror + hierarchy_mirror_order(ctx), ctx->h_order.size() * sizeof(uint32_t));
    uint32_t count[BUILD_LEVELS + 1];
    memcpy(count, ctx->hb_mirror + hierarchy_mirror_counts(ctx), sizeof(count));
    /* the level table is the deepest level first (drt_build_kernels.h), as tree_maps lays it out */
    ctx->level_first.assign(1, 0u);
    ctx->hb_depth = 1;
    for (uint32_t l = BUILD_LEVELS; l >= 1; l -= 1)
    {
        if (count[l] == 0u) continue;
        ctx->hb_depth = std::max(ctx->hb_depth, l + 1u);
        ctx->level_first.push_back(ctx->level_first.back() + count[l]);
    }
    ctx->hb_mirror_pending = false;
    return 0;
}

static int hierarchy_check(const drt_context *ctx, uint32_t flags, const char *name)
{
    if (!ctx) return fail(-1, "%s: ctx is null", name);
    if (flags != 0u) return fail(-1, "%s: unknown flags 0x%x", name, flags);
    return 0;
}

/* a level's size is the device's to know: the grid is sized by its bound, min(2^level, m / 2) items, and strides over what is there */
static uint32_t hierarchy_level_grid(uint32_t m, uint32_t level)
{
    const uint32_t bound = std::min<uint32_t>(level < 31u ? 1u << level : 0x80000000u, m / 2u);
    return (std::max(bound, 1u) + BUILD_BLOCK - 1) / BUILD_BLOCK;
}

/* The three stages of a build that need no scene, each on buffers it is given: hierarchy_enqueue runs them on the context's, the
 * selftests (drt_selftest_build_sort, drt_selftest_build_topology) on scratch of their own. Nothing else launches these kernels. */

/* the status words and the root item: before the bounds pass and before the topology */
static int hierarchy_enqueue_init(hipStream_t st, const BuildTables &bt, uint4 *items0)
{
    hipLaunchKernelGGL(drt_build_init_kernel, dim3(1), dim3(64), 0, st, bt, items0);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* the sort of m (key, payload) pairs in keys[0], pos[0], in place: keys[1], pos[1] ([m] each) and table ([SORT_DIGITS][tiles]) are its
 * temporaries, and the result ends where it began because SORT_PASSES is even */
static int hierarchy_enqueue_sort(hipStream_t st, uint64_t *const keys[2], uint32_t *const pos[2], uint32_t *table, uint32_t m)
{
    const uint32_t n_tiles = (m + SORT_TILE - 1) / SORT_TILE;
    for (uint32_t pass = 0; pass < SORT_PASSES; pass += 1)
    {
        const int from = (int)(pass & 1u), to = 1 - from;
        hipLaunchKernelGGL(drt_build_count_kernel, dim3(n_tiles), dim3(BUILD_BLOCK), 0, st, keys[from], m, pass * 8u, table, n_tiles);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(drt_build_scan_kernel, dim3(1), dim3(SORT_DIGITS), 0, st, table, n_tiles);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(drt_build_scatter_kernel, dim3(n_tiles), dim3(BUILD_BLOCK), 0, st, keys[from], pos[from], keys[to], pos[to], m, pass * 8u, table, n_tiles);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

/* the links of the tree over tt.m >= 2 sorted keys, level by level: tt.level_count and items[0] as hierarchy_enqueue_init left them,
 * items[0] and items[1] ([m / 2 + 1] each) the lists of two neighbouring levels in turn */
static int hierarchy_enqueue_topology(hipStream_t st, const TopologyTables &tt, uint4 *const items[2])
{
    const uint32_t deepest = hierarchy_max_level(tt.m);
    for (uint32_t level = 0; level <= deepest; level += 1) /* top down; a kernel boundary between two levels */
    {
        hipLaunchKernelGGL(drt_build_topology_kernel, dim3(hierarchy_level_grid(tt.m, level)), dim3(BUILD_BLOCK), 0, st, tt, items[level & 1u], items[1u - (level & 1u)], level);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

static int hierarchy_enqueue(drt_context *ctx)
{
    if (!ctx->use_bvh) return 0; /* nothing to build: as DRT_SURFACES_REBUILD there */
    int rc = hierarchy_prepare(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t m = (uint32_t)ctx->h_order.size();
    if (m >= 2u) /* (the trees over no surface and over one are the two special roots the context has) */
    {
        HIP_TRY(hipEventRecord(ctx->hb_ev[0], st));
        if (!ctx->boxes_valid && (rc = update_enqueue_derive(ctx))) return rc; /* no update yet: the boxes and the extent word are not made */
        const uint32_t grid = (m + BUILD_BLOCK - 1) / BUILD_BLOCK;
        BuildTables bt;
        bt.boxes = ctx->d_boxes;
        bt.tree_surf = ctx->d_hb_tree_surf;
        bt.bounds = (unsigned long long *)ctx->d_hb_status.get();
        bt.level_count = (uint32_t *)(ctx->d_hb_status + BUILD_BOUND_WORDS * 8);
        bt.m = m;
        if ((rc = hierarchy_enqueue_init(st, bt, ctx->d_hb_items[0]))) return rc;
        hipLaunchKernelGGL(drt_build_bounds_kernel, dim3(grid), dim3(BUILD_BLOCK), 0, st, bt);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(drt_build_keys_kernel, dim3(grid), dim3(BUILD_BLOCK), 0, st, bt, ctx->d_hb_keys[0], ctx->d_hb_pos[0]);
        HIP_TRY(hipGetLastError());
        uint64_t *const keys[2] = {ctx->d_hb_keys[0], ctx->d_hb_keys[1]};
        uint32_t *const pos[2] = {ctx->d_hb_pos[0], ctx->d_hb_pos[1]};
        uint4 *const items[2] = {ctx->d_hb_items[0], ctx->d_hb_items[1]};
        if ((rc = hierarchy_enqueue_sort(st, keys, pos, ctx->d_hb_table, m))) return rc;
        TopologyTables tt;
        tt.keys = ctx->d_hb_keys[0];
        tt.pos = ctx->d_hb_pos[0];
        tt.tree_surf = ctx->d_hb_tree_surf;
        tt.surf_type = ctx->dsc.surf_type;
        tt.nodes = const_cast<BvhNode *>(ctx->dsc.bvh_nodes);
        tt.leaf = const_cast<BvhLeafPrim *>(ctx->dsc.bvh_leaf);
        tt.leaf_parent = ctx->d_leaf_parent;
        tt.order = ctx->d_hb_order;
        tt.levels = ctx->d_levels;
        tt.level_count = bt.level_count;
        tt.m = m;
        if ((rc = hierarchy_enqueue_topology(st, tt, items))) return rc;
        const LeafTables lt = update_leaf_tables(ctx);
        hipLaunchKernelGGL(drt_bvh_leaf_kernel, dim3((m + UPDATE_BLOCK - 1) / UPDATE_BLOCK), dim3(UPDATE_BLOCK), 0, st, lt, m, ctx->cam_reach);
        HIP_TRY(hipGetLastError());
        for (uint32_t level = hierarchy_max_level(m); level >= 1u; level -= 1) /* deepest first */
        {
            hipLaunchKernelGGL(drt_build_refit_kernel, dim3(hierarchy_level_grid(m, level)), dim3(BUILD_BLOCK), 0, st, tt.nodes, ctx->d_levels, bt.level_count, m, level);
            HIP_TRY(hipGetLastError());
        }
    }
    ctx->hb_timed = false;
    ctx->hb_ms = 0.0; /* (no kernels: no time) */
    if (m >= 2u)
    {
        HIP_TRY(hipEventRecord(ctx->hb_ev[1], st));
        ctx->hb_timed = true;
        /* the host's copy, on its way behind the build: whoever needs it waits for hb_ev[2] (hierarchy_adopt) */
        HIP_TRY(hipMemcpyAsync(ctx->hb_mirror, ctx->dsc.bvh_nodes, hierarchy_mirror_order(ctx), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ctx->hb_mirror + hierarchy_mirror_order(ctx), ctx->d_hb_order, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ctx->hb_mirror + hierarchy_mirror_counts(ctx), ctx->d_hb_status + BUILD_BOUND_WORDS * 8, (BUILD_LEVELS + 1) * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(ctx->hb_ev[2], st));
        ctx->hb_mirror_pending = true;
    }
    ctx->hb_builds += 1;
    ctx->win_dirty = true; /* (the live window is worked out again: from the host's surfaces, where those are current) */
    ctx->hb_built_by = 1;
    ctx->refits = 0;
    return 0;
}

extern "C" int drt_rebuild_hierarchy(drt_context *ctx, uint32_t flags)
{
    g_last_error.clear();
    int rc = hierarchy_check(ctx, flags, "drt_rebuild_hierarchy");
    if (rc) return rc;
    return hierarchy_enqueue(ctx);
}

extern "C" int drt_group_rebuild_hierarchy(drt_group *g, uint32_t flags)
{
    g_last_error.clear();
    if (!g) return fail(-1, "drt_group_rebuild_hierarchy: the group is null");
    int rc = 0;
    for (drt_context *c : g->ctx)
        if (c && (rc = hierarchy_check(c, flags, "drt_group_rebuild_hierarchy"))) return rc;
    for (drt_context *c : g->ctx)
        if (c && c->use_bvh && (rc = hierarchy_prepare(c))) return rc; /* what can fail, before any context changes */
    for (drt_context *c : g->ctx)
        if (c && (rc = hierarchy_enqueue(c))) return rc;
    return 0;
}

extern "C" int drt_get_hierarchy_report(drt_context *ctx, drt_hierarchy_report *out)
{
    g_last_error.clear();
    if (!ctx || !out) return fail(-1, "drt_get_hierarchy_report: null argument");
    memset(out, 0, sizeof(*out));
    if (!ctx->use_bvh) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->hb_timed)
    {
        float ms = 0.0f;
        HIP_TRY(hipEventSynchronize(ctx->hb_ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, ctx->hb_ev[0], ctx->hb_ev[1]));
        ctx->hb_ms = (double)ms;
        ctx->hb_timed = false;
    }
    int rc = hierarchy_adopt(ctx);
    if (rc) return rc;
    out->nodes = (uint32_t)ctx->h_nodes.size();
    out->leaf_surfaces = (uint32_t)ctx->h_order.size();
    out->depth = ctx->hb_depth;
    out->device_builds = ctx->hb_builds;
    out->built_by = ctx->hb_built_by;
    out->kernel_ms = ctx->hb_ms;
    return 0;
}

extern "C" int drt_read_hierarchy(drt_context *ctx, void *nodes, uint32_t n_nodes, uint32_t *leaf_surface, uint32_t n_leaf)
{
    g_last_error.clear();
    if (!ctx) return fail(-1, "drt_read_hierarchy: ctx is null");
    if (!ctx->use_bvh) return fail(-1, "drt_read_hierarchy: the context has no hierarchy (its scene is scanned out of LDS)");
    if (n_nodes != ctx->h_nodes.size() || n_leaf != ctx->h_order.size())
        return fail(-1, "drt_read_hierarchy: room for %u nodes and %u leaf slots, the tree has %zu and %zu", n_nodes, n_leaf, ctx->h_nodes.size(), ctx->h_order.size());
    if (!nodes || (n_leaf > 0 && !leaf_surface)) return fail(-1, "drt_read_hierarchy: null argument");
    int rc = hierarchy_adopt(ctx);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    /* the boxes are the device's business after an update or a device build: the nodes come from there */
    HIP_TRY(hipMemcpy(nodes, ctx->dsc.bvh_nodes, (size_t)n_nodes * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (n_leaf) memcpy(leaf_surface, ctx->h_order.data(), (size_t)n_leaf * sizeof(uint32_t));
    return 0;
}

extern "C" int drt_render_tile_multi(const drt_scene *scene, const drt_camera *camera, const drt_params *params,
                                     const int32_t *devices, uint32_t n_devices, double *dst_pixels, double *dst_avgs,
                                     double *dst_vars, drt_stats *stats)
{
    g_last_error.clear();
    const bool xyz = params && params->mode == DRT_MODE_XYZ;
    if (!dst_pixels || (!xyz && (!dst_avgs || !dst_vars))) return fail(-1, "null film buffer");
    if (xyz) dst_avgs = dst_vars = nullptr;
    drt_group *g = drt_group_create(scene, camera, params, devices, n_devices);
    if (!g) return -1;
    int rc = 0;
    do
    {
        if (!(params->flags & DRT_FLAG_FILM_ZERO) && (rc = drt_group_write_film(g, dst_pixels, dst_avgs, dst_vars))) break;
        if ((rc = drt_group_render(g, params->first_sample, params->spp))) break;
        if ((rc = drt_group_read_film(g, dst_pixels, dst_avgs, dst_vars))) break;
        if (stats && (rc = drt_group_get_stats(g, stats))) break;
    } while (0);
    drt_group_destroy(g);
    return rc;
}

extern "C" int drt_selftest_path_ids(int device, const uint64_t *bases, uint32_t n_draws, const uint32_t *steps, uint32_t n_steps, uint32_t n_samples,
                                     uint32_t tile_w, uint64_t *out)
{
    g_last_error.clear();
    if (!bases || !steps || !out || n_draws == 0 || n_steps == 0 || n_samples == 0 || tile_w == 0) return fail(-1, "drt_selftest_path_ids: empty argument");
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_steps; k += 1)
    {
        if (steps[k] == 0 || steps[k] > 64) return fail(-1, "drt_selftest_path_ids: step %u is %u, not in 1..64", k, steps[k]);
        total += steps[k];
    }
    if (total > (1u << 20) || total * n_draws > (1u << 24)) return fail(-1, "drt_selftest_path_ids: too many ids");
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint64_t> d_bases, d_out;
    DevBuf<uint32_t> d_steps;
    const size_t out_bytes = (size_t)total * n_draws * 4 * 8;
    HIP_TRY(d_bases.need(n_draws));
    HIP_TRY(d_steps.need(n_steps));
    HIP_TRY(d_out.need(out_bytes / 8));
    HIP_TRY(hipMemcpy(d_bases, bases, (size_t)n_draws * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_steps, steps, (size_t)n_steps * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(drt_path_id_kernel, dim3(n_draws), dim3(64), 0, 0, d_bases, d_steps, n_steps, (uint32_t)total, n_samples, tile_w, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_selftest_arith(int device, int op, const double *a, const double *b, double *out, uint64_t n)
{
    g_last_error.clear();
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> da, db, dout;
    size_t out_n = (op == 2) ? 2 * n : n;
    HIP_TRY(da.need(n));
    HIP_TRY(db.need(n));
    HIP_TRY(dout.need(out_n));
    HIP_TRY(hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, b, n * 8, hipMemcpyHostToDevice));
    Event e0, e1;
    HIP_TRY(e0.need());
    HIP_TRY(e1.need());
    HIP_TRY(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(drt_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, da, db, dout, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipDeviceSynchronize());
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (getenv("DRT_VERBOSE")) fprintf(stderr, "drt_selftest_arith op %d n %llu: %.3f ms\n", op, (unsigned long long)n, ms);
    HIP_TRY(hipMemcpy(out, dout, out_n * 8, hipMemcpyDeviceToHost));
    return 0;
}

#define BUILD_SELFTEST_MAX (1u << 24) /* elements: far above any test, far below where an index would wrap */
#define BUILD_SELFTEST_GUARD 64u      /* elements in front of and behind every array the sort writes */

extern "C" int drt_selftest_build_sort(int device, const uint64_t *keys, uint32_t m, uint64_t *keys_out, uint32_t *pos_out)
{
    g_last_error.clear();
    if (!keys || !keys_out || !pos_out) return fail(-1, "drt_selftest_build_sort: null argument");
    if (m == 0u || m > BUILD_SELFTEST_MAX) return fail(-1, "drt_selftest_build_sort: %u keys, not in 1..%u", m, BUILD_SELFTEST_MAX);
    for (uint32_t k = 0; k < m; k += 1)
        if (keys[k] > BUILD_KEY_UNBOUNDED) return fail(-1, "drt_selftest_build_sort: key %u has bit 63 set", k);
    HIP_TRY(hipSetDevice(device));
    /* both halves of the double buffer between guard words: a scatter outside [0, m) is reported, not left to chance */
    const size_t G = BUILD_SELFTEST_GUARD, room = (size_t)m + 2 * G;
    const uint64_t key_guard = 0xA5A5A5A5A5A5A5A5ull;
    const uint32_t pos_guard = 0xA5A5A5A5u;
    std::vector<uint64_t> hk(room, key_guard);
    std::vector<uint32_t> hp(room, pos_guard);
    DevBuf<uint64_t> dk[2];
    DevBuf<uint32_t> dp[2], d_table;
    uint64_t *d_keys[2];
    uint32_t *d_pos[2];
    for (int k = 0; k < 2; k += 1)
    {
        HIP_TRY(dk[k].need(room));
        HIP_TRY(dp[k].need(room));
        HIP_TRY(hipMemcpy(dk[k], hk.data(), room * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dp[k], hp.data(), room * sizeof(uint32_t), hipMemcpyHostToDevice));
        d_keys[k] = dk[k] + G;
        d_pos[k] = dp[k] + G;
    }
    HIP_TRY(d_table.need((size_t)SORT_DIGITS * ((m + SORT_TILE - 1) / SORT_TILE)));
    for (uint32_t k = 0; k < m; k += 1) hp[G + k] = k; /* the payload drt_build_keys_kernel writes: the position */
    HIP_TRY(hipMemcpy(d_keys[0], keys, (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_pos[0], hp.data() + G, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice));
    int rc = hierarchy_enqueue_sort(0, d_keys, d_pos, d_table, m);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < 2; k += 1)
    {
        HIP_TRY(hipMemcpy(hk.data(), dk[k], room * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hp.data(), dp[k], room * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t g = 0; g < G; g += 1)
            if (hk[g] != key_guard || hk[G + m + g] != key_guard || hp[g] != pos_guard || hp[G + m + g] != pos_guard)
                return fail(-3, "drt_selftest_build_sort: buffer %d was written outside its %u elements", k, m);
    }
    HIP_TRY(hipMemcpy(keys_out, d_keys[0], (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pos_out, d_pos[0], (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_selftest_live_resources(uint64_t out[4])
{
    g_last_error.clear();
    if (!out) return fail(-1, "drt_selftest_live_resources: null argument");
    out[0] = DeviceMem::live();
    out[1] = PinnedMem::live();
    out[2] = Event::live();
    out[3] = Stream::live();
    return 0;
}

extern "C" int drt_selftest_build_topology(int device, const uint64_t *sorted_keys, uint32_t m, int32_t *child, int32_t *count, uint32_t *level_count,
                                           uint32_t *levels_out)
{
    g_last_error.clear();
    if (!sorted_keys || !child || !count || !level_count || (m > 2u && !levels_out)) return fail(-1, "drt_selftest_build_topology: null argument");
    if (m < 2u || m > BUILD_SELFTEST_MAX) return fail(-1, "drt_selftest_build_topology: %u keys, not in 2..%u (a build launches nothing below 2)", m, BUILD_SELFTEST_MAX);
    for (uint32_t k = 0; k < m; k += 1)
        if (sorted_keys[k] > BUILD_KEY_UNBOUNDED || (k > 0u && sorted_keys[k - 1] > sorted_keys[k]))
            return fail(-1, "drt_selftest_build_topology: key %u is out of order or has bit 63 set", k);
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint64_t> d_keys;
    DevBuf<uint32_t> d_same, d_type, d_leaf_parent, d_order;
    DevBuf<BvhNode> d_nodes;
    DevBuf<BvhLeafPrim> d_leaf;
    DevBuf<uint2> d_levels;
    DevBuf<uint4> d_items[2];
    DevBuf<unsigned char> d_status;
    HIP_TRY(d_keys.need(m));
    HIP_TRY(d_same.need(m));
    HIP_TRY(d_type.need(m));
    HIP_TRY(d_leaf_parent.need(m));
    HIP_TRY(d_order.need(m));
    HIP_TRY(d_nodes.need((size_t)m - 1));
    HIP_TRY(d_leaf.need(m));
    HIP_TRY(d_levels.need((size_t)m - 2));
    for (int k = 0; k < 2; k += 1) HIP_TRY(d_items[k].need((size_t)m / 2 + 1)); /* as hierarchy_prepare sizes them */
    HIP_TRY(d_status.need(BUILD_STATUS_BYTES));
    std::vector<uint32_t> same(m), type(m, (uint32_t)DRT_GEO_SPHERE);
    for (uint32_t k = 0; k < m; k += 1) same[k] = k; /* tree_surf and pos are identities: slot j holds surface j */
    HIP_TRY(hipMemcpy(d_keys, sorted_keys, (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_same, same.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_type, type.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_nodes, 0xFF, ((size_t)m - 1) * sizeof(BvhNode)));
    HIP_TRY(hipMemset(d_levels, 0xFF, std::max<size_t>((size_t)m - 2, 1) * sizeof(uint2)));
    BuildTables bt;
    bt.boxes = nullptr; /* no bounds pass, no keys pass: nothing reads it */
    bt.tree_surf = d_same;
    bt.bounds = (unsigned long long *)d_status.get();
    bt.level_count = (uint32_t *)(d_status + BUILD_BOUND_WORDS * 8);
    bt.m = m;
    TopologyTables tt;
    tt.keys = d_keys;
    tt.pos = d_same;
    tt.tree_surf = d_same;
    tt.surf_type = d_type;
    tt.nodes = d_nodes;
    tt.leaf = d_leaf;
    tt.leaf_parent = d_leaf_parent;
    tt.order = d_order;
    tt.levels = d_levels;
    tt.level_count = bt.level_count;
    tt.m = m;
    int rc = hierarchy_enqueue_init(0, bt, d_items[0]);
    uint4 *const items[2] = {d_items[0], d_items[1]};
    if (rc || (rc = hierarchy_enqueue_topology(0, tt, items))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<BvhNode> nodes((size_t)m - 1);
    HIP_TRY(hipMemcpy(nodes.data(), d_nodes, nodes.size() * sizeof(BvhNode), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nodes.size(); i += 1)
        for (int c = 0; c < 2; c += 1)
        {
            child[2 * i + c] = nodes[i].child[c];
            count[2 * i + c] = nodes[i].count[c];
        }
    HIP_TRY(hipMemcpy(level_count, bt.level_count, (BUILD_LEVELS + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (m > 2u) HIP_TRY(hipMemcpy(levels_out, d_levels, ((size_t)m - 2) * sizeof(uint2), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_selftest_unit(int device, int func, const double *in, uint32_t in_stride, double *out, uint32_t out_stride, uint64_t n)
{
    g_last_error.clear();
    if (func < 0 || func >= DRT_UNIT_COUNT) return fail(-1, "unknown unit function %d", func);
    if (!in || !out || in_stride == 0 || out_stride == 0) return fail(-1, "null argument");
    /* what each function reads and writes per record: a caller with narrower records would make the kernel read past its buffers */
    static const uint32_t need_in[DRT_UNIT_COUNT] = {10, 18, 6, 8, 6, 1, 1, 7, 10, 3, 4, 1, 12, 20, 12};
    static const uint32_t need_out[DRT_UNIT_COUNT] = {1, 1, 3, 3, 9, 4, 4, 1, 1, 1, 1, 2, 1, 1, 2};
    if (in_stride < need_in[func] || out_stride < need_out[func])
        return fail(-1, "unit function %d needs %u doubles in and %u out per record", func, need_in[func], need_out[func]);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> din, dout;
    HIP_TRY(din.need(n * in_stride));
    HIP_TRY(dout.need(n * out_stride));
    HIP_TRY(hipMemcpy(din, in, n * in_stride * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dout, 0, n * out_stride * 8));
    hipLaunchKernelGGL(drt_unit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, func, din, in_stride, dout, out_stride, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, n * out_stride * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int drt_selftest_division(int device, int func, const double *in, uint32_t in_stride, double *out, uint32_t out_stride, uint64_t n)
{
    g_last_error.clear();
    if (func < 0 || func >= DRT_DIVISION_COUNT) return fail(-1, "unknown division function %d", func);
    if (!in || !out) return fail(-1, "null argument");
    /* as in drt_selftest_unit: narrower records would make the kernel read or write past its buffers */
    static const uint32_t need_in[DRT_DIVISION_COUNT] = {DRT_DIVISION_SHARED_IN, DRT_DIVISION_DRAW_IN};
    static const uint32_t need_out[DRT_DIVISION_COUNT] = {DRT_DIVISION_SHARED_OUT, DRT_DIVISION_DRAW_OUT};
    if (in_stride < need_in[func] || out_stride < need_out[func])
        return fail(-1, "division function %d needs %u doubles in and %u out per record", func, need_in[func], need_out[func]);
    if (n == 0) return 0;
    if (n > BUILD_SELFTEST_MAX) return fail(-1, "drt_selftest_division: %llu records, more than %u", (unsigned long long)n, BUILD_SELFTEST_MAX);
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> din, dout;
    HIP_TRY(din.need(n * in_stride));
    HIP_TRY(dout.need(n * out_stride));
    HIP_TRY(hipMemcpy(din, in, n * in_stride * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dout, 0, n * out_stride * 8));
    hipLaunchKernelGGL(drt_division_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, func, din, in_stride, dout, out_stride, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, n * out_stride * 8, hipMemcpyDeviceToHost));
    return 0;
}

/* Fresnel kind of a BDSF: 0 none, 1 dielectric, 2 conductor (build_device_scene's fresnel_kind, one function) */
static int bdsf_fresnel_kind(uint32_t b)
{
    if (b == DRT_BDSF_fs_dielectric_reflectance_bdsf || b == DRT_BDSF_fs_dielectric_transmittance_bdsf) return 1;
    if (b == DRT_BDSF_fs_conductor_bdsf || b == DRT_BDSF_ct_conductor_bdsf) return 2;
    return 0;
}

/* the override tables of drt_material_kernel: the context's material table with every list replaced by one BDSF (copies 0-6) or
 * every dir_func by another (copies 7-12). A one-function list needs what that function needs; its pair rows are kept only when the
 * function is of the kind the rows were tabulated for (never read a dielectric's rel_sq row as a conductor's cA, cB), else PAIR_NONE. */
static int material_variants(drt_context *ctx)
{
    int rc = spectra_read_back(ctx);
    if (rc) return rc;
    if (ctx->d_mat_variants && !ctx->variants_stale) return 0;
    const uint32_t n_mat = ctx->dsc.n_mat;
    std::vector<DevMaterial> v((size_t)DRT_MAT_VARIANTS * n_mat);
    for (uint32_t k = 0; k < (uint32_t)DRT_MAT_VARIANTS; k += 1)
        for (uint32_t m = 0; m < n_mat; m += 1)
        {
            DevMaterial dm = ctx->host_mats[m];
            if (k < (uint32_t)DRT_NUM_BDSFS)
            {
                memset(dm.bdsfs, 0, sizeof(dm.bdsfs));
                dm.bdsfs[0] = k;
                dm.num_bdsfs = 1;
                dm.bdsf_packed = k;
                dm.needs = bdsf_needs(k);
                dm.vertex_flags = 0;
                const int rows = dm.pair_out == PAIR_NONE ? 0 : (dm.pair_out & PAIR_CONDUCTOR) ? 2 : 1;
                if (rows == 0 || rows != bdsf_fresnel_kind(k)) dm.pair_out = dm.pair_in = PAIR_NONE;
            }
            else dm.dir_func = k - (uint32_t)DRT_NUM_BDSFS;
            v[(size_t)k * n_mat + m] = dm;
        }
    if (!ctx->d_mat_variants) /* after a material update: the same allocation, made again */
    {
        DevBuf<unsigned char> buf;
        HIP_TRY(buf.need(v.size() * sizeof(DevMaterial)));
        ctx->d_mat_variants = (DevMaterial *)(unsigned char *)buf;
        ctx->allocations.push_back(std::move(buf));
    }
    HIP_TRY(hipMemcpy(ctx->d_mat_variants, v.data(), v.size() * sizeof(DevMaterial), hipMemcpyHostToDevice));
    ctx->variants_stale = false;
    return 0;
}

extern "C" int drt_selftest_material(drt_context *ctx, int func, const double *in, uint32_t in_stride, double *out, uint32_t out_stride,
                                     uint64_t n)
{
    g_last_error.clear();
    if (!ctx || !in || !out) return fail(-1, "null argument");
    if (func < 0 || func >= DRT_MAT_COUNT) return fail(-1, "unknown material function %d", func);
    const uint32_t S = ctx->dsc.S, n_mat = ctx->dsc.n_mat;
    const uint32_t need_in = func == DRT_MAT_EVALUATE ? DRT_MAT_EVAL_IN : DRT_MAT_SAMPLE_IN;
    const uint32_t need_out = func == DRT_MAT_EVALUATE ? S + 1u : DRT_MAT_SAMPLE_OUT;
    if (in_stride < need_in || out_stride < need_out)
        return fail(-1, "material function %d needs %u doubles in and %u out per record", func, need_in, need_out);
    /* every index the kernel follows is checked here, so that no record makes it read outside the scene's tables */
    auto index_ok = [](double x, double lo, double hi) { return x >= lo && x < hi && x == (double)(int64_t)x; };
    for (uint64_t r = 0; r < n; r += 1)
    {
        const double *a = in + r * in_stride;
        for (int k = 10; k < 13; k += 1)
            if (!index_ok(a[k], 0.0, (double)n_mat)) return fail(-1, "record %llu: material index %g (the scene has %u)", (unsigned long long)r, a[k], n_mat);
        const DevMaterial &sm = ctx->host_mats[(uint32_t)a[10]];
        if (func == DRT_MAT_EVALUATE)
        {
            if (!index_ok(a[13], -1.0, (double)DRT_NUM_BDSFS)) return fail(-1, "record %llu: unknown bdsf id %g", (unsigned long long)r, a[13]);
            if (!index_ok(a[17], 0.0, 4.0)) return fail(-1, "record %llu: unknown mode %g", (unsigned long long)r, a[17]);
            if ((uint32_t)a[17] & DRT_MAT_MODE_SIMPLE)
            {
                bool fresnel = a[13] >= 0.0 ? bdsf_fresnel_kind((uint32_t)a[13]) != 0 : false;
                for (uint32_t j = 0; a[13] < 0.0 && j < sm.num_bdsfs; j += 1) fresnel = fresnel || bdsf_fresnel_kind(sm.bdsfs[j]) != 0;
                if (fresnel) return fail(-1, "record %llu: the SIMPLE instantiation has no Fresnel functions", (unsigned long long)r);
            }
        }
        else
        {
            if (!index_ok(a[13], -1.0, (double)DRT_NUM_DIRFS)) return fail(-1, "record %llu: unknown dir_func id %g", (unsigned long long)r, a[13]);
            if (a[13] < 0.0 && sm.dir_func >= (uint32_t)DRT_NUM_DIRFS)
                return fail(-1, "record %llu: material %u has no direction sampler (dir_func %u)", (unsigned long long)r, (uint32_t)a[10], sm.dir_func);
        }
    }
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = material_variants(ctx);
    if (rc) return rc;
    DevBuf<double> din, dout;
    HIP_TRY(din.need(n * in_stride));
    HIP_TRY(dout.need(n * out_stride));
    HIP_TRY(hipMemcpy(din, in, n * in_stride * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dout, 0, n * out_stride * 8));
    hipLaunchKernelGGL(drt_material_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ctx->dsc, ctx->d_mat_variants, func, din, in_stride,
                       dout, out_stride, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, n * out_stride * 8, hipMemcpyDeviceToHost));
    return 0;
}
