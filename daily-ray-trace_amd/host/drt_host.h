/*
 * drt_host.h -- the POSIX C host of the MI355X build: the part of daily-ray-trace that stays on
 * the CPU (config + .scn reading, SPD tables, scene/camera build, .spd writing) and hands the
 * per-pixel loop to libdrt_hip.so through include/drt_hip.h.
 *
 * Mirrors, with the same names and argument meaning:
 *   config_arguments / render_image()   src/daily_ray_trace.h:28-55, :177; src/daily_ray_trace.c:635
 *   parse_config()                      src/read_scene.c:604-765
 *   parse_scene() (superset grammar)    src/read_scene.c:345-602
 *   load_csv_file_to_spectrum()         src/read_scene.c:801-872
 *   init_spd_tables / rgb_f64_to_spectrum / generate_blackbody_spectrum   src/spectrum.c
 *   init_camera / init_scene / init_spd src/daily_ray_trace.c:49-211
 *   win32_platform.c file/timer/alloc   -> POSIX (calloc, stdio, clock_gettime)
 */
#ifndef DRT_HOST_H
#define DRT_HOST_H

#include <stdint.h>
#include "../../include/drt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef uint8_t  u8;
typedef uint32_t u32;
typedef uint64_t u64;
typedef double   f64;

typedef enum
{
    FILM_SAMPLE_NONE,
    FILM_SAMPLE_CENTER,
    FILM_SAMPLE_RANDOM,
    FILM_SAMPLE_COUNT
} film_sample_scheme;

/* Same fields, order and sizes as the reference's config_arguments (1136 bytes). */
typedef struct
{
    u32  num_pixel_samples;
    u32  max_cast_depth;
    u32  output_width;
    u32  output_height;
    f64  min_wl;
    f64  max_wl;
    f64  wl_interval;
    char input_scene[64];
    char output_spd[64];
    char average_spd[64];
    char variance_spd[64];
    char output_bmp[64];
    char average_bmp[64];
    char variance_bmp[64];
    char white_spd[64];
    char cmf_x[64];
    char cmf_y[64];
    char cmf_z[64];
    char red_spd[64];
    char green_spd[64];
    char blue_spd[64];
    char cyan_spd[64];
    char magenta_spd[64];
    char yellow_spd[64];
    film_sample_scheme pixel_scheme;
} config_arguments;

/* .spd header, src/daily_ray_trace.h:59-68 (40 bytes) */
typedef struct
{
    u32 id;
    u32 width_in_pixels;
    u32 height_in_pixels;
    u32 number_of_wavelengths;
    u32 has_filter_values;
    f64 min_wavelength;
    f64 wavelength_interval;
} spd_file_header;

/* Host extras that the reference has no field for (device choice, RNG seed, batch size, adaptive sampling);
 * read from the environment by render_image(): DRT_DEVICE, DRT_DEVICES, DRT_SEED, DRT_BATCH_SPP, DRT_CHECKPOINT_SPP, DRT_RESUME,
 * DRT_ADAPTIVE_ERROR, DRT_ADAPTIVE_MIN_SPP, DRT_ADAPTIVE_STEP, DRT_ADAPTIVE_FLOOR, DRT_ADAPTIVE_CHECKPOINT_ROUNDS, DRT_ADAPTIVE_RESUME,
 * DRT_DENOISE_K, DRT_DENOISE_RADIUS, DRT_DENOISE_PATCH, DRT_DENOISE_ALPHA, DRT_DENOISE_SPD, DRT_DENOISE_VAR_SPD, DRT_FEATURES*, DRT_MATTES, DRT_PICK,
 * DRT_PROJECTION, DRT_ORTHO_WIDTH, DRT_TURNTABLE, DRT_LIGHT_LEVELS, DRT_DEPTH_CUTS, DRT_REGIONS, DRT_SENSOR, DRT_BUCKETS, DRT_LOBES. */
#define DRT_HOST_MAX_PICKS 64
#define DRT_HOST_MAX_LEVELS 64
#define DRT_HOST_MAX_REGIONS 64
typedef struct
{
    int32_t  device;
    uint64_t seed;
    uint32_t batch_spp;
    uint32_t quiet;
    uint32_t checkpoint_spp; /* rewrite the .spd files every this many samples (0: only at the end) */
    uint32_t resume;         /* continue from the .spd files of an earlier (checkpointed) run */
    uint32_t n_devices;      /* > 0: render on devices[0..n_devices) at once, image rows dealt cyclically (drt_group_*); */
    int32_t  devices[16];    /* 0: the single `device` above. DRT_DEVICES="0,1,2,3" or "all" (every visible device) */
    uint32_t all_devices;
    /* adaptive sampling (drt_group_render_adaptive) when adaptive != 0: num_pixel_samples is max_spp; the .spd filter column holds
     * each pixel's sample count. Not combined with checkpoint_spp or resume: an adaptive render has checkpoints of its own, */
    uint32_t adaptive, adaptive_min_spp, adaptive_step;
    double   adaptive_error, adaptive_floor;
    uint32_t adaptive_checkpoint_rounds; /* written after every this many rendering rounds (0: none), */
    uint32_t adaptive_resume;            /* and continues from one (or from a uniform render's), every pixel from the count it holds */
    /* the variance-guided denoiser (drt_group_denoise) when denoise != 0: the finished film, uniform, adaptive or resumed, is filtered
     * into two more .spd files (the average file's header); the three standard outputs stay byte for byte what they are without it */
    uint32_t denoise, denoise_radius, denoise_patch;
    double   denoise_k, denoise_alpha;
    char     denoise_spd[256], denoise_var_spd[256];
    /* the first-hit feature buffers (drt_group_render_features, every pixel at the count its film holds) when features != 0: mean and m2 as
     * two 8-"wavelength" .spd files without a filter column, and <output_spd>.normal.bmp / .depth.bmp / .coverage.bmp; the three standard
     * outputs and the denoiser's files stay byte for byte what they are without it */
    uint32_t features;
    char     features_spd[256], features_m2_spd[256];
    /* the ID mattes (drt_group_render_mattes, every pixel at the count its film holds) when mattes != 0: <output_spd>.surface_id.spd and
     * .material_id.spd, 12 channels per pixel ((double)id_0, count_0 / c, ..., id_5, count_5 / c in rank order, an empty slot -1, 0),
     * the previews <output_spd>.surface_id.bmp and .material_id.bmp, and <output_spd>.mattes.txt, which names every surface and
     * material; every other output stays byte for byte what it is without it */
    uint32_t mattes;
    /* DRT_PICK: what is under these pixels (drt_group_cast_pixels after the render): one `pick` line per entry on stdout; every output
     * file stays byte for byte what it is without it */
    uint32_t n_picks;
    uint32_t pick_xy[DRT_HOST_MAX_PICKS][2], pick_sample[DRT_HOST_MAX_PICKS];
    /* DRT_PROJECTION: the scene through another projection than the configured camera's (a ray table bound before the first sample,
     * drt_group_bind_rays): 0 the camera, DRT_HOST_PROJECTION_EQUIRECT, DRT_HOST_PROJECTION_ORTHO with ortho_width (DRT_ORTHO_WIDTH).
     * Checkpoints, resuming and the adaptive forms work as with the camera; not combined with features, mattes or picks, which ask
     * for the camera's rays */
    uint32_t projection;
    double   ortho_width;
    /* DRT_TURNTABLE=n: n frames from ONE context or group, frame k through drt_host_turntable_camera(k, n): per frame one drt_reset_film,
     * one drt_set_camera and the render the configuration asks for (uniform or adaptive); frame k writes the three standard outputs with
     * .%04u before the extension. Not combined with checkpoints, resuming, DRT_PROJECTION or the post-passes (denoiser, features, mattes,
     * picks). 0: off, and everything as without it */
    uint32_t turntable;
    /* DRT_LIGHT_LEVELS="k0,k1,...": one frame per level from ONE group: per frame one drt_group_reset_film, one drt_group_update_spectra
     * that gives every row an emissive material names as its emission the scene's own row times k (one multiplication per sample, on
     * the host), and the render the configuration asks for; frame j writes the three standard outputs with .%04u before the extension.
     * Not combined with DRT_TURNTABLE or with what the turntable is not combined with. 0 levels: off, and everything as without it */
    uint32_t n_levels;
    double   levels[DRT_HOST_MAX_LEVELS];
    /* DRT_DEPTH_CUTS="d0,d1,...": beside the render, its film at every shorter max_cast_depth listed (drt_group_bind_depth_cuts: ascending
     * whole numbers from 1 to max_cast_depth, DRT_MAX_DEPTH_CUTS at most): per cut d the three standard .spd outputs again as
     * <output_spd>.depth<d>.spd, <average_spd>.depth<d>.spd, <variance_spd>.depth<d>.spd and the picture <output_spd>.depth<d>.bmp; every
     * other output stays byte for byte what it is without it. Not combined with adaptive sampling, checkpoints or resuming, DRT_TURNTABLE
     * or DRT_LIGHT_LEVELS. 0 cuts: off */
    uint32_t n_depth_cuts;
    uint32_t depth_cuts[DRT_MAX_DEPTH_CUTS];
    /* DRT_REGIONS="x,y,w,h:spp;...": a sample map (drt_group_render_sample_map) of num_pixel_samples everywhere and, inside a region
     * (clipped to the image), the largest spp of the regions that cover the pixel. The three standard outputs through the standard
     * writer, and <output_spd>.counts.bmp: every pixel's count over the largest, as a grey picture. Not combined with adaptive sampling,
     * checkpoints or resuming, DRT_TURNTABLE, DRT_LIGHT_LEVELS, DRT_DEPTH_CUTS or DRT_PROJECTION. 0 regions: off */
    uint32_t n_regions;
    uint32_t regions[DRT_HOST_MAX_REGIONS][5]; /* x, y, w, h, spp */
    /* DRT_SENSOR="r.csv,g.csv,b.csv": a sensor film (drt_group_bind_sensor) of one channel per file, DRT_MAX_SENSOR_CHANNELS at most,
     * every curve resampled on the render's grid by drt_host_csv_to_spectrum: the three standard outputs again with n channels as
     * <output_spd>.sensor.spd, <average_spd>.sensor.spd and <variance_spd>.sensor.spd, and with exactly three curves the picture
     * <output_spd>.sensor.bmp through the identity matrix; every other output stays byte for byte what it is without it. Not combined
     * with adaptive sampling, checkpoints or resuming, DRT_TURNTABLE, DRT_LIGHT_LEVELS, DRT_DEPTH_CUTS or DRT_REGIONS. 0 curves: off */
    uint32_t n_sensor;
    char     sensor_csv[DRT_MAX_SENSOR_CHANNELS][256];
    /* DRT_BUCKETS="n[,trim]": bucket films (drt_group_bind_buckets) of n buckets, DRT_MAX_BUCKETS at most: per bucket b the three standard
     * .spd outputs again as <output_spd>.bucket<b>.spd, <average_spd>.bucket<b>.spd and <variance_spd>.bucket<b>.spd, and with n >= 2 the
     * resolve (drt_group_resolve_buckets with `trim`; the median's, (n - 1) / 2, when none is given): the estimate as
     * <average_spd>.robust.spd, the error as <variance_spd>.robust.spd, both under the average file's header, and the picture of the
     * estimate <output_spd>.robust.bmp; every other output stays byte for byte what it is without it. Not combined with adaptive
     * sampling, checkpoints or resuming, DRT_TURNTABLE, DRT_LIGHT_LEVELS, DRT_DEPTH_CUTS, DRT_SENSOR or DRT_REGIONS. 0 buckets: off */
    uint32_t n_buckets, bucket_trim;
    /* DRT_LOBES=standard|functions: lobe films (drt_group_bind_lobes) with that preset's map: per film k the three standard .spd outputs
     * again as <output_spd>.lobe<k>.spd, <average_spd>.lobe<k>.spd and <variance_spd>.lobe<k>.spd, the picture of its mean
     * <output_spd>.lobe<k>.bmp, and <output_spd>.lobes.txt, one line "<k> <name>" per film; every other output stays byte for byte what
     * it is without it. Not combined with DRT_BUCKETS or anything DRT_BUCKETS is not combined with. 0 films: off */
    uint32_t n_lobes;
    drt_lobe_map lobe_map;
    const char *const *lobe_names;
} drt_host_options;
#define DRT_HOST_PROJECTION_EQUIRECT 1u
#define DRT_HOST_PROJECTION_ORTHO 2u

/* the `adaptive` line of a version-3 checkpoint manifest: what the film was rendered with so far */
typedef struct { uint32_t min_spp, max_spp, step; double rel_error, floor; } drt_host_adaptive_line;

/* Fills *config from the text of a config.cfg. Unknown keys are fatal (exit(-1)), like the reference.
 * Paths may use '\' or '/'. */
void parse_config(char *config_contents, u32 config_contents_size, config_arguments *config);
void print_config_arguments(config_arguments *config);

/* The drop-in: same signature as the reference. Writes the three .spd files. */
void render_image(config_arguments *config);
/* Same, with explicit options and statistics; returns 0 on success. */
int render_image_ex(config_arguments *config, const drt_host_options *opt, drt_stats *stats);

/* A loaded scene: owns every array the drt_scene/drt_camera inside point to. */
typedef struct drt_host_scene drt_host_scene;

typedef struct
{
    const char *white, *cmf_x, *cmf_y, *cmf_z, *rgb_red, *rgb_green, *rgb_blue, *rgb_cyan, *rgb_magenta, *rgb_yellow;
} spd_tables_csvs;

/*
 * init_spd_tables + load_scene in one call. `spectra_dir` is the directory `csv <file>` material
 * entries are looked up in (the reference hard-codes "spectra\\", src/daily_ray_trace.c:93).
 * tables==NULL uses <spectra_dir>/{white_rgb_to_spd,cmf_x,...}.csv.
 * Returns NULL and sets drt_host_last_error() when a file is missing; grammar errors exit(-1).
 */
drt_host_scene *drt_host_load_scene(const char *scene_path, const char *spectra_dir, const spd_tables_csvs *tables,
                                    u32 width_px, u32 height_px, f64 min_wl, f64 max_wl, f64 wl_interval);
/* Same from memory (the text of a .scn). */
drt_host_scene *drt_host_load_scene_text(const char *scene_text, u32 scene_size, const char *spectra_dir,
                                         const spd_tables_csvs *tables, u32 width_px, u32 height_px,
                                         f64 min_wl, f64 max_wl, f64 wl_interval);
void              drt_host_free_scene(drt_host_scene *s);
const drt_scene  *drt_host_scene_data(const drt_host_scene *s);
const drt_camera *drt_host_camera_data(const drt_host_scene *s);
const char       *drt_host_material_name(const drt_host_scene *s, u32 i);
const char       *drt_host_surface_name(const drt_host_scene *s, u32 i);
const char       *drt_host_last_error(void);

/* Standalone pieces, exported for the parity tests. */
/* load_csv_file_to_spectrum: resample a CSV onto the grid; returns 1, or 0 if the file is missing. */
u32  drt_host_csv_to_spectrum(const char *csv_path, f64 min_wl, f64 wl_interval, u32 num_samples, f64 *dst);
/* rgb_f64_to_spectrum with the 7 rgb tables given as [7][num_samples] (white,red,green,blue,cyan,magenta,yellow). */
void drt_host_rgb_to_spectrum(const f64 *rgb_tables, u32 num_samples, const f64 rgb[3], f64 *dst);
void drt_host_blackbody_spectrum(f64 min_wl, f64 wl_interval, u32 num_samples, f64 temperature, f64 *dst);
/* init_camera: fills *camera from position/target/roll/fov/fdepth/flength/aperture and the image size. */
void drt_host_init_camera(drt_camera *camera, const f64 position[3], const f64 target[3], f64 roll, f64 fov,
                          f64 fdepth, f64 flength, f64 aperture, u32 width_px, u32 height_px);
/* The camera of frame k of an n-frame turntable (DRT_TURNTABLE, drt_set_camera): the scene's own camera with its position turned by
 * 360 k / n degrees about the axis through its target along the up direction drt_host_init_camera starts from, (0, 1, 0), made by
 * drt_host_init_camera itself. k = 0 is the scene's camera bit for bit. Returns 0, or -1 (nothing written) for a null pointer, n = 0 or
 * an empty image. */
int drt_host_turntable_camera(const drt_host_scene *s, u32 width_px, u32 height_px, u32 k, u32 n, drt_camera *out);

/* Ray tables for drt_bind_rays (include/drt_hip.h), one layer, [height][width][3] each, row 0 at the bottom as the film's rows are.
 * Both return 0, or -1 (nothing written) for a null pointer, an empty image or a film_width that is not a finite number above 0.
 * equirect: every origin is the camera's aperture_position; pixel (x, y) looks along longitude ((x + 0.5) / width - 0.5) * 2 pi (towards
 * `right`) and latitude ((y + 0.5) / height - 0.5) * pi (towards `up`) about `forward`, as a unit vector: the centre of an image of odd
 * width and height looks along `forward`.
 * ortho: every direction is `forward` as it stands; the origins lie on the rectangle of film_width x film_width * height / width,
 * spanned by `right` and `up`, whose centre is the aperture_position, at the pixels' centres. */
int drt_host_rays_equirect(const drt_camera *camera, u32 width, u32 height, f64 *origins, f64 *dirs);
int drt_host_rays_ortho(const drt_camera *camera, u32 width, u32 height, f64 film_width, f64 *origins, f64 *dirs);

/* Name tables expanded from include/bdsf_list.h (same role as bdsf_name_list / dir_func_name_list). */
extern const char *bdsf_name_list[];
extern const u32   num_bdsfs_defined;
extern const char *dir_func_name_list[];
extern const u32   num_dir_funcs_defined;

/* .spd files */
int drt_host_write_spd(const char *path, u32 width, u32 height, u32 num_wl, u32 has_filter, f64 min_wl, f64 interval,
                       const f64 *pixels);
/* Reads a .spd; *pixels is malloc'ed. Returns 0 on success. */
int drt_host_read_spd(const char *path, spd_file_header *header, f64 **pixels);

/* The outputs of render_image() as one crash-safe set (host/drt_checkpoint.c): the three .spd files, with
 * with_raw_variance also <variance_spd>.raw and the manifest <output_spd>.ckpt a resumed run needs. Returns 0 on success. */
int drt_host_write_outputs(const config_arguments *config, u32 width, u32 height, u32 S, f64 min_wl, f64 interval,
                           const f64 *dst_pixels, const f64 *dst_avgs, const f64 *dst_vars, int with_raw_variance,
                           u32 samples_done, u64 seed);
/* Loads a checkpointed set into the (caller-allocated, full-frame) film buffers if, and only if, manifest, headers, file
 * sizes, filter sums and means all agree with each other and with the job; returns 0 and the samples held, or nonzero
 * (buffers then hold garbage: clear them) with the reason in drt_host_checkpoint_error(). */
int drt_host_load_checkpoint(const config_arguments *config, u32 width, u32 height, u32 S, u64 seed, f64 *dst_pixels,
                             f64 *dst_avgs, f64 *dst_vars, u32 *samples_done);
/* The adaptive forms. Writing: the same set under a version-3 manifest (`samples` = the largest count of any pixel, one `adaptive`
 * line). Loading: a version-3 or a version-2 manifest; every pixel's filter sum a whole number from 2 to the job's num_pixel_samples,
 * the largest the manifest's `samples`, and mean = sum / the pixel's own count on a spread of pixels. *line (may be NULL) gets the
 * manifest's adaptive line, zeros from version 2. */
int drt_host_write_outputs_adaptive(const config_arguments *config, u32 width, u32 height, u32 S, f64 min_wl, f64 interval,
                                    const f64 *dst_pixels, const f64 *dst_avgs, const f64 *dst_vars, int with_raw_variance,
                                    u64 seed, const drt_host_adaptive_line *adaptive);
int drt_host_load_checkpoint_adaptive(const config_arguments *config, u32 width, u32 height, u32 S, u64 seed, f64 *dst_pixels,
                                      f64 *dst_avgs, f64 *dst_vars, u32 *largest_count, drt_host_adaptive_line *line);
/* The projection of the job that writes or loads checkpoints from here on (drt_host_options.projection and ortho_width; 0: the camera).
 * It enters the manifest's scene fingerprint, so a checkpoint rendered through the camera or another projection is not resumed under
 * this one. render_image_ex sets it from its options. */
void drt_host_checkpoint_projection(u32 projection, f64 ortho_width);
const char *drt_host_checkpoint_error(void);

/* .spd -> BMP post-process (spd_file_to_bmp, src/win32_main.c:115-121). cmf: [4][S] rows rw, x, y, z. */
void drt_host_spectrum_to_rgb(const f64 *cmf, u32 S, f64 interval, const f64 *spd, f64 rgb[3]);
int  drt_host_write_bmp(const char *path, u32 width, u32 height, const f64 *rgb);
int  drt_host_write_bmp_bgra(const char *path, u32 width, u32 height, const u8 *bgra);
/* One feature of a [n][8] feature mean as BMP pixel bytes: drt_read_feature_bgra's rule (include/drt_hip.h) on the host. */
void drt_host_feature_bgra(const f64 *mean, u64 n, int which, f64 lo, f64 hi, u8 *bgra);
/* One layer of the ID mattes ([n][2][6] ids and counts, [n][4] tail) as BMP pixel bytes: drt_read_matte_bgra's rule on the host. */
void drt_host_matte_bgra(const int32_t *ids, const u32 *counts, const u32 *tail, u64 n, int layer, u8 *bgra);
int  drt_host_spd_file_to_bmp(const char *spd_path, const char *bmp_path, const f64 *cmf);

#ifdef __cplusplus
}
#endif
#endif
