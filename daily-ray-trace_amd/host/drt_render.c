/*
 * drt_render.c -- render_image() for the POSIX + HIP host (replaces src/daily_ray_trace.c:635-777).
 *
 * Same inputs (config_arguments) and outputs (three .spd files, then the three BMPs of the reference's
 * main()). The `for sample / for y / for x` loop (src/daily_ray_trace.c:710-745) is the C-ABI launcher
 * (include/drt_hip.h: drt_group_create / drt_group_render / drt_group_read_film, the session form of
 * drt_render_tile over one or several GPUs, so the film can stay on the device between checkpoints); everything around it stays plain C.
 * There is no CPU fallback: if the launcher fails, render_image reports it and exits.
 */
#include "drt_host.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static f64 now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (f64)ts.tv_sec * 1000.0 + (f64)ts.tv_nsec * 1e-6;
}

/* a .spd without a filter column, written under a temporary name and moved into place */
static int publish_spd(const char *path, u32 width, u32 height, u32 S, f64 min_wl, f64 interval, const f64 *data)
{
    char tmp[300];
    if (snprintf(tmp, sizeof(tmp), "%s.tmp", path) >= (int)sizeof(tmp)) return -1;
    if (drt_host_write_spd(tmp, width, height, S, 0, min_wl, interval, data) != 0) return -1;
    return rename(tmp, path) == 0 ? 0 : -1;
}

#define MATTE_CHANNELS (DRT_MATTE_LAYERS * DRT_MATTE_SLOTS) /* ids and counts per pixel; also the doubles per pixel of a layer's .spd */

/* The ID mattes' files, each by temporary name + rename: <base>.surface_id.spd and <base>.material_id.spd (12 channels per pixel:
 * (double)id_k, count_k / c in rank order), the two previews beside them, and <base>.mattes.txt with the names behind the ids. */
static int publish_mattes(const char *base, const drt_host_scene *hs, u32 width, u32 height, const int32_t *ids, const u32 *counts, const u32 *tail)
{
    static const char *const layer_name[DRT_MATTE_LAYERS] = { "surface_id", "material_id" };
    const drt_scene *scene = drt_host_scene_data(hs);
    const u64 num_pixels = (u64)width * height;
    char path[300], tmp[304];
    f64 *chan = (f64 *)malloc(num_pixels * MATTE_CHANNELS * sizeof(f64));
    u8 *fb = (u8 *)malloc(num_pixels * 4 + 4);
    int bad = (!chan || !fb) ? -1 : 0;
    for (int y = 0; !bad && y < DRT_MATTE_LAYERS; y += 1)
    {
        for (u64 px = 0; px < num_pixels; px += 1)
        {
            const u64 at = (px * DRT_MATTE_LAYERS + (u64)y) * DRT_MATTE_SLOTS;
            const f64 c = (f64)tail[px * 4];
            for (int k = 0; k < DRT_MATTE_SLOTS; k += 1)
            {
                chan[px * MATTE_CHANNELS + 2 * k] = (f64)ids[at + k];
                chan[px * MATTE_CHANNELS + 2 * k + 1] = (f64)counts[at + k] / c;
            }
        }
        if (snprintf(path, sizeof(path), "%s.%s.spd", base, layer_name[y]) >= (int)sizeof(path)) { bad = -1; break; }
        if (publish_spd(path, width, height, MATTE_CHANNELS, scene->min_wavelength, scene->wavelength_interval, chan) != 0) { bad = -1; break; }
        snprintf(path, sizeof(path), "%s.%s.bmp", base, layer_name[y]);
        snprintf(tmp, sizeof(tmp), "%s.tmp", path);
        drt_host_matte_bgra(ids, counts, tail, num_pixels, y, fb);
        if (drt_host_write_bmp_bgra(tmp, width, height, fb) != 0 || rename(tmp, path) != 0) bad = -1;
    }
    free(fb);
    free(chan);
    if (bad) return bad;
    if (snprintf(path, sizeof(path), "%s.mattes.txt", base) >= (int)sizeof(path)) return -1;
    snprintf(tmp, sizeof(tmp), "%s.tmp", path);
    FILE *f = fopen(tmp, "w");
    if (!f) return -1;
    for (u32 i = 0; i < scene->num_surfaces; i += 1)
        fprintf(f, "surface %u %s material %u\n", i, drt_host_surface_name(hs, i), scene->surfaces[i].material);
    for (u32 i = 0; i < scene->num_materials; i += 1) fprintf(f, "material %u %s\n", i, drt_host_material_name(hs, i));
    bad = ferror(f);
    if (fclose(f) != 0 || bad) return -1;
    return rename(tmp, path) == 0 ? 0 : -1;
}

/* "out.spd" -> "out.0003.spd" (no extension: the number goes at the end); -1 when the name does not fit the field */
static int frame_path(char dst[64], const char *src, u32 frame)
{
    if (!src[0]) { dst[0] = 0; return 0; }
    const char *dot = strrchr(src, '.'), *slash = strrchr(src, '/');
    if (dot && slash && dot < slash) dot = NULL;
    const int stem = dot ? (int)(dot - src) : (int)strlen(src);
    return snprintf(dst, 64, "%.*s.%04u%s", stem, src, frame, dot ? dot : "") < 64 ? 0 : -1;
}

/* DRT_DEPTH_CUTS: "<src>.depth<d><ext>" into a config field; -1 when it does not fit */
static int depth_path(char dst[64], const char *src, u32 depth, const char *ext)
{
    return snprintf(dst, 64, "%s.depth%u%s", src, depth, ext) < 64 ? 0 : -1;
}

/* DRT_SENSOR: "<src>.sensor<ext>" into a config field; -1 when it does not fit */
static int sensor_path(char dst[64], const char *src, const char *ext)
{
    return snprintf(dst, 64, "%s.sensor%s", src, ext) < 64 ? 0 : -1;
}

/* DRT_BUCKETS: "<src>.bucket<b><ext>" and "<src>.robust<ext>" into a config field; -1 when it does not fit */
static int bucket_path(char dst[64], const char *src, u32 b, const char *ext)
{
    return snprintf(dst, 64, "%s.bucket%u%s", src, b, ext) < 64 ? 0 : -1;
}
static int robust_path(char dst[64], const char *src, const char *ext)
{
    return snprintf(dst, 64, "%s.robust%s", src, ext) < 64 ? 0 : -1;
}

/* DRT_LOBES: "<src>.lobe<k><ext>" and "<src>.lobes.txt" into a config field; -1 when it does not fit */
static int lobe_path(char dst[64], const char *src, u32 k, const char *ext)
{
    return snprintf(dst, 64, "%s.lobe%u%s", src, k, ext) < 64 ? 0 : -1;
}
static int lobes_txt_path(char dst[64], const char *src)
{
    return snprintf(dst, 64, "%s.lobes.txt", src) < 64 ? 0 : -1;
}

/* Frame k of DRT_LIGHT_LEVELS: `rows` gets the scene's rows [*first_row, *first_row + *count) -- from the first to the last row an emissive
 * material names as its emission -- with every such row times `level` (one multiplication per sample) and the rows between as they are.
 * No emissive material: *count = 0. */
static void light_level_rows(const drt_scene *scene, f64 level, f64 *rows, u32 *first_row, u32 *count)
{
    const u32 S = scene->num_wavelengths;
    u32 lo = 0xFFFFFFFFu, hi = 0;
    for (u32 m = 0; m < scene->num_materials; m += 1)
        if (scene->materials[m].is_emissive && scene->materials[m].emission_spd >= 0)
        {
            const u32 r = (u32)scene->materials[m].emission_spd;
            if (r < lo) lo = r;
            if (r > hi) hi = r;
        }
    *first_row = 0;
    *count = 0;
    if (lo == 0xFFFFFFFFu) return;
    *first_row = lo;
    *count = hi - lo + 1;
    memcpy(rows, scene->spds + (size_t)lo * S, (size_t)*count * S * sizeof(f64));
    for (u32 r = lo; r <= hi; r += 1)
    {
        int names_it = 0;
        for (u32 m = 0; m < scene->num_materials && !names_it; m += 1)
            names_it = scene->materials[m].is_emissive && scene->materials[m].emission_spd == (int32_t)r;
        if (!names_it) continue;
        for (u32 i = 0; i < S; i += 1) rows[(size_t)(r - lo) * S + i] = scene->spds[(size_t)r * S + i] * level;
    }
}

/* DRT_TURNTABLE=n: n frames from one group, the second and every later one at the price of a drt_set_camera instead of a drt_group_create.
 * DRT_LIGHT_LEVELS: one frame per level from one group through the scene's own camera, at the price of a drt_group_update_spectra */
static int render_turntable(config_arguments *config, const drt_host_options *opt, drt_stats *stats_out)
{
    const u32 width = config->output_width, height = config->output_height, frames = opt->turntable ? opt->turntable : opt->n_levels;
    const char *const mode_name = opt->turntable ? "DRT_TURNTABLE" : "DRT_LIGHT_LEVELS";
    spd_tables_csvs csvs;
    csvs.white = config->white_spd;  csvs.cmf_x = config->cmf_x;      csvs.cmf_y = config->cmf_y;
    csvs.cmf_z = config->cmf_z;      csvs.rgb_red = config->red_spd;  csvs.rgb_green = config->green_spd;
    csvs.rgb_blue = config->blue_spd; csvs.rgb_cyan = config->cyan_spd; csvs.rgb_magenta = config->magenta_spd;
    csvs.rgb_yellow = config->yellow_spd;
    char spectra_dir[128];
    snprintf(spectra_dir, sizeof(spectra_dir), "%s", config->white_spd);
    char *slash = strrchr(spectra_dir, '/');
    if (slash) *slash = 0; else snprintf(spectra_dir, sizeof(spectra_dir), "spectra");
    for (u32 k = 0; k < frames; k += 1)
    {
        config_arguments fc = *config;
        if (frame_path(fc.output_spd, config->output_spd, k) || frame_path(fc.average_spd, config->average_spd, k) ||
            frame_path(fc.variance_spd, config->variance_spd, k) || frame_path(fc.output_bmp, config->output_bmp, k) ||
            frame_path(fc.average_bmp, config->average_bmp, k) || frame_path(fc.variance_bmp, config->variance_bmp, k))
        {
            fprintf(stderr, "render_image: %s: an output name with .%04u before its extension is longer than 63 characters\n", mode_name, k);
            return -1;
        }
    }
    drt_host_scene *hs = drt_host_load_scene(config->input_scene, spectra_dir, &csvs, width, height, config->min_wl, config->max_wl, config->wl_interval);
    if (!hs)
    {
        fprintf(stderr, "render_image: %s\n", drt_host_last_error());
        return -1;
    }
    const drt_scene *scene = drt_host_scene_data(hs);
    const u32 S = scene->num_wavelengths;
    const u64 num_pixels = (u64)width * height;
    f64 *dst_pixels = (f64 *)calloc(num_pixels * (S + 1), sizeof(f64));
    f64 *dst_avgs = (f64 *)calloc(num_pixels * S, sizeof(f64));
    f64 *dst_vars = (f64 *)calloc(num_pixels * S, sizeof(f64));
    u8 *bgra = (u8 *)malloc(num_pixels * 4 + 4);
    f64 *level_rows = opt->n_levels ? (f64 *)malloc((size_t)scene->num_spds * S * sizeof(f64) + 8) : NULL;
    if (!dst_pixels || !dst_avgs || !dst_vars || !bgra || (opt->n_levels && !level_rows))
    {
        fprintf(stderr, "render_image: out of memory for %llu pixels\n", (unsigned long long)num_pixels);
        return -1;
    }
    drt_params p;
    memset(&p, 0, sizeof(p));
    p.width = width;
    p.height = height;
    p.tile_w = width;
    p.tile_h = height;
    p.row_stride = 1;
    p.spp = config->num_pixel_samples;
    p.max_depth = config->max_cast_depth;
    p.pixel_scheme = (u32)config->pixel_scheme;
    p.seed = opt->seed;
    p.mode = DRT_MODE_SPECTRAL;
    p.device = opt->device;
    p.batch_spp = opt->batch_spp;
    drt_host_checkpoint_projection(0, 0.0);
    int32_t one_device = p.device;
    const int32_t *devices = &one_device;
    u32 n_devices = 1;
    if (opt->all_devices) { devices = NULL; n_devices = 0; }
    else if (opt->n_devices) { devices = opt->devices; n_devices = opt->n_devices; }
    drt_stats stats;
    memset(&stats, 0, sizeof(stats));
    int rc = 0, wrc = 0;
    drt_group *ctx = drt_group_create(scene, drt_host_camera_data(hs), &p, devices, n_devices);
    if (!ctx) rc = -1;
    if (!rc && !opt->quiet && drt_group_size(ctx) > 1) printf("Rendering on %u devices\n", drt_group_size(ctx));
    for (u32 k = 0; !rc && !wrc && k < frames; k += 1)
    {
        const f64 t0 = now_ms();
        config_arguments fc = *config;
        frame_path(fc.output_spd, config->output_spd, k);
        frame_path(fc.average_spd, config->average_spd, k);
        frame_path(fc.variance_spd, config->variance_spd, k);
        frame_path(fc.output_bmp, config->output_bmp, k);
        frame_path(fc.average_bmp, config->average_bmp, k);
        frame_path(fc.variance_bmp, config->variance_bmp, k);
        if (opt->turntable)
        {
            drt_camera cam;
            if (drt_host_turntable_camera(hs, width, height, k, frames, &cam) != 0) { rc = -1; break; }
            if ((rc = drt_group_reset_film(ctx))) break;
            if ((rc = drt_group_set_camera(ctx, &cam))) break;
        }
        else
        {
            u32 first_row = 0, count = 0;
            light_level_rows(scene, opt->levels[k], level_rows, &first_row, &count);
            if ((rc = drt_group_reset_film(ctx))) break;
            if ((rc = drt_group_update_spectra(ctx, level_rows, first_row, count, 0))) break;
        }
        if (opt->adaptive)
        {
            drt_adaptive a;
            memset(&a, 0, sizeof(a));
            a.min_spp = opt->adaptive_min_spp;
            a.max_spp = p.spp;
            a.step = opt->adaptive_step;
            a.rel_error = opt->adaptive_error;
            a.floor = opt->adaptive_floor;
            if ((rc = drt_group_render_adaptive(ctx, &a))) break;
        }
        else if ((rc = drt_group_render(ctx, 0, p.spp))) break;
        if ((rc = drt_group_read_film(ctx, dst_pixels, dst_avgs, dst_vars))) break;
        if ((rc = drt_group_get_stats(ctx, &stats))) break;
        wrc = drt_host_write_outputs(&fc, width, height, S, scene->min_wavelength, scene->wavelength_interval, dst_pixels, dst_avgs, dst_vars, 0, p.spp, p.seed);
        if (wrc) { fprintf(stderr, "render_image: %s\n", drt_host_checkpoint_error()); break; }
        const char *bmp_path[3] = { fc.output_bmp, fc.average_bmp, fc.variance_bmp };
        for (int b = 0; !rc && !wrc && b < 3 && fc.output_bmp[0]; b += 1)
        {
            if (!bmp_path[b][0]) continue;
            if ((rc = drt_group_read_bgra(ctx, b, bgra))) break;
            if (drt_host_write_bmp_bgra(bmp_path[b], width, height, bgra) != 0)
            {
                fprintf(stderr, "render_image: could not write one of the .bmp outputs\n");
                wrc = -1;
            }
        }
        if (!rc && !wrc && !opt->quiet)
            printf("Frame %u / %u: %fms (device %fms: trace %fms, shade+film %fms)\n", k + 1, frames, now_ms() - t0, stats.total_ms, stats.trace_ms, stats.shade_ms);
    }
    if (rc) fprintf(stderr, "render_image: the HIP launcher failed (%d): %s\n", rc, drt_last_error());
    if (ctx) drt_group_destroy(ctx);
    if (stats_out) *stats_out = stats;
    free(level_rows);
    free(bgra);
    free(dst_vars);
    free(dst_avgs);
    free(dst_pixels);
    drt_host_free_scene(hs);
    return rc ? rc : (wrc ? -2 : 0);
}

int render_image_ex(config_arguments *config, const drt_host_options *opt, drt_stats *stats_out)
{
    if (opt && (opt->turntable || opt->n_levels)) return render_turntable(config, opt, stats_out);
    u32 width = config->output_width, height = config->output_height;
    spd_tables_csvs csvs;
    csvs.white = config->white_spd;  csvs.cmf_x = config->cmf_x;      csvs.cmf_y = config->cmf_y;
    csvs.cmf_z = config->cmf_z;      csvs.rgb_red = config->red_spd;  csvs.rgb_green = config->green_spd;
    csvs.rgb_blue = config->blue_spd; csvs.rgb_cyan = config->cyan_spd; csvs.rgb_magenta = config->magenta_spd;
    csvs.rgb_yellow = config->yellow_spd;

    /* material `csv` entries live next to the table CSVs (the reference hard-codes "spectra\") */
    char spectra_dir[128];
    snprintf(spectra_dir, sizeof(spectra_dir), "%s", config->white_spd);
    char *slash = strrchr(spectra_dir, '/');
    if (slash) *slash = 0; else snprintf(spectra_dir, sizeof(spectra_dir), "spectra");

    drt_host_scene *hs = drt_host_load_scene(config->input_scene, spectra_dir, &csvs, width, height,
                                             config->min_wl, config->max_wl, config->wl_interval);
    if (!hs)
    {
        fprintf(stderr, "render_image: %s\n", drt_host_last_error());
        return -1;
    }
    const drt_scene *scene = drt_host_scene_data(hs);
    u32 S = scene->num_wavelengths;
    u64 num_pixels = (u64)width * height;

    /* zero-filled accumulators (VirtualAlloc semantics, src/daily_ray_trace.c:689-691), 64-bit sizes */
    f64 *dst_pixels = (f64 *)calloc(num_pixels * (S + 1), sizeof(f64));
    f64 *dst_avgs = (f64 *)calloc(num_pixels * S, sizeof(f64));
    f64 *dst_vars = (f64 *)calloc(num_pixels * S, sizeof(f64));
    if (!dst_pixels || !dst_avgs || !dst_vars)
    {
        fprintf(stderr, "render_image: out of memory for %llu pixels\n", (unsigned long long)num_pixels);
        return -1;
    }

    drt_params p;
    memset(&p, 0, sizeof(p));
    p.width = width;
    p.height = height;
    p.tile_w = width;
    p.tile_h = height;
    p.row_stride = 1;
    p.spp = config->num_pixel_samples;
    p.max_depth = config->max_cast_depth;
    p.pixel_scheme = (u32)config->pixel_scheme;
    p.seed = opt ? opt->seed : 1;
    p.mode = DRT_MODE_SPECTRAL;
    p.device = opt ? opt->device : 0;
    p.batch_spp = opt ? opt->batch_spp : 0;

    /*
     * Progressive accumulation (the reference only sketches it, src/daily_ray_trace.c:620-633): the
     * film lives on the device for the whole render; every `checkpoint_spp` samples the three .spd files are
     * rewritten, plus the un-normalised variance (<variance_spd>.raw) that a resumed run needs. A resumed run
     * (opt->resume) reloads those files, takes the number of samples done from the filter sum, and continues --
     * bit-identical to an uninterrupted run, because sample k always uses the same per-path seeds.
     */
    drt_host_checkpoint_projection(opt ? opt->projection : 0, opt ? opt->ortho_width : 0.0); /* a checkpoint belongs to its projection */
    drt_stats stats;
    memset(&stats, 0, sizeof(stats));
    u32 done = 0;
    const u64 seed = p.seed;
    if (opt && opt->resume)
    {
        /* host/drt_checkpoint.c: accepted only when manifest, headers, sizes, filter sums and means agree with the job */
        if (drt_host_load_checkpoint(config, width, height, S, seed, dst_pixels, dst_avgs, dst_vars, &done) == 0)
        {
            if (!(opt && opt->quiet)) printf("Resuming after %u samples\n", done);
        }
        else
        {
            fprintf(stderr, "render_image: not resuming (%s), starting at sample 0\n", drt_host_checkpoint_error());
            memset(dst_pixels, 0, num_pixels * (S + 1) * sizeof(f64));
            memset(dst_avgs, 0, num_pixels * S * sizeof(f64));
            memset(dst_vars, 0, num_pixels * S * sizeof(f64));
            done = 0;
        }
    }
    f64 t0 = now_ms();
    int rc = 0;
    /* one device, or several at once with the image rows dealt cyclically over them (one host thread, drt_group_*) */
    int32_t one_device = p.device;
    const int32_t *devices = &one_device;
    u32 n_devices = 1;
    if (opt && opt->all_devices) { devices = NULL; n_devices = 0; }
    else if (opt && opt->n_devices) { devices = opt->devices; n_devices = opt->n_devices; }
    /* DRT_SENSOR: every curve on the render's grid, before the first device call */
    const u32 n_sensor = opt ? opt->n_sensor : 0;
    f64 *sensor_curves = NULL;
    if (n_sensor)
    {
        sensor_curves = (f64 *)calloc((size_t)n_sensor * S, sizeof(f64));
        if (!sensor_curves) rc = -3;
        for (u32 k = 0; !rc && k < n_sensor; k += 1)
            if (!drt_host_csv_to_spectrum(opt->sensor_csv[k], scene->min_wavelength, scene->wavelength_interval, S, sensor_curves + (size_t)k * S))
            {
                fprintf(stderr, "render_image: DRT_SENSOR: cannot read %s\n", opt->sensor_csv[k]);
                rc = -1;
            }
    }
    drt_group *ctx = rc ? NULL : drt_group_create(scene, drt_host_camera_data(hs), &p, devices, n_devices);
    if (!ctx && !rc) rc = -1;
    if (!rc && !(opt && opt->quiet) && drt_group_size(ctx) > 1) printf("Rendering on %u devices\n", drt_group_size(ctx));
    /* DRT_PROJECTION: the first rays from a table, bound while the film is still without samples (a resumed film is written after it) */
    if (!rc && opt && opt->projection)
    {
        f64 *ray_o = (f64 *)malloc(num_pixels * 3 * sizeof(f64)), *ray_d = (f64 *)malloc(num_pixels * 3 * sizeof(f64));
        if (!ray_o || !ray_d) rc = -3;
        if (!rc)
            rc = opt->projection == DRT_HOST_PROJECTION_EQUIRECT ? drt_host_rays_equirect(drt_host_camera_data(hs), width, height, ray_o, ray_d)
                                                                 : drt_host_rays_ortho(drt_host_camera_data(hs), width, height, opt->ortho_width, ray_o, ray_d);
        if (!rc)
        {
            drt_ray_table table;
            memset(&table, 0, sizeof(table));
            table.origins = ray_o;
            table.dirs = ray_d;
            table.n_layers = 1;
            rc = drt_group_bind_rays(ctx, &table);
        }
        free(ray_d);
        free(ray_o);
    }
    /* DRT_DEPTH_CUTS: the cut films, bound while the film is still without samples */
    if (!rc && opt && opt->n_depth_cuts) rc = drt_group_bind_depth_cuts(ctx, opt->depth_cuts, opt->n_depth_cuts);
    /* DRT_SENSOR: the sensor film, bound while the film is still without samples */
    if (!rc && n_sensor) rc = drt_group_bind_sensor(ctx, sensor_curves, n_sensor);
    /* DRT_BUCKETS: the bucket films, bound while the film is still without samples */
    if (!rc && opt && opt->n_buckets) rc = drt_group_bind_buckets(ctx, opt->n_buckets);
    /* DRT_LOBES: the lobe films, bound while the film is still without samples */
    if (!rc && opt && opt->n_lobes) rc = drt_group_bind_lobes(ctx, opt->n_lobes, &opt->lobe_map);
    if (!rc && done) rc = drt_group_write_film(ctx, dst_pixels, dst_avgs, dst_vars);
    if (!rc && opt && opt->adaptive && (opt->adaptive_checkpoint_rounds || opt->adaptive_resume))
    {
        /* An adaptive render that can be taken up again: samples [0, min_spp) of every pixel as a uniform render, then
         * drt_group_render_adaptive_continue in slices of adaptive_checkpoint_rounds rounds -- the same render as drt_group_render_adaptive
         * (include/drt_hip.h) -- with a checkpoint after each slice. A resumed run adopts the checkpoint's film instead of rendering the
         * first samples, every pixel at the count it holds; continuing with a tighter DRT_ADAPTIVE_ERROR or more num_pixel_samples
         * gives the film of one render with those. */
        const drt_host_adaptive_line line = { opt->adaptive_min_spp, p.spp, opt->adaptive_step, opt->adaptive_error, opt->adaptive_floor };
        u32 rounds = 0, at_max = 0, largest = 0;
        u64 paths = 0;
        int resumed = 0;
        if (opt->adaptive_resume)
        {
            if (drt_host_load_checkpoint_adaptive(config, width, height, S, seed, dst_pixels, dst_avgs, dst_vars, &largest, NULL) == 0)
            {
                u64 held = 0;
                for (u64 px = 0; px < num_pixels; px += 1) held += (u64)dst_pixels[px * (S + 1) + S];
                resumed = 1;
                if (!opt->quiet) printf("Resuming an adaptive render: %llu pixels hold %llu samples, %u at most\n", (unsigned long long)num_pixels, (unsigned long long)held, largest);
                rc = drt_group_write_film(ctx, dst_pixels, dst_avgs, dst_vars);
            }
            else fprintf(stderr, "render_image: not resuming (%s), starting at sample 0\n", drt_host_checkpoint_error());
        }
        if (!rc && !resumed)
        {
            rc = drt_group_render(ctx, 0, opt->adaptive_min_spp);
            rounds = 1;
            paths = (u64)opt->adaptive_min_spp * num_pixels;
        }
        for (u32 left = 1; !rc && left;)
        {
            drt_adaptive a;
            memset(&a, 0, sizeof(a));
            a.min_spp = 2; /* not used by the continuation */
            a.max_spp = p.spp;
            a.step = opt->adaptive_step;
            a.rel_error = opt->adaptive_error;
            a.floor = opt->adaptive_floor;
            if ((rc = drt_group_render_adaptive_continue(ctx, &a, opt->adaptive_checkpoint_rounds, &left))) break;
            rounds += a.rounds;
            paths += a.paths;
            at_max = a.pixels_at_max;
            if (left) /* a checkpoint: the final write below uses the same code */
            {
                if ((rc = drt_group_read_film(ctx, dst_pixels, dst_avgs, dst_vars))) break;
                if (drt_host_write_outputs_adaptive(config, width, height, S, scene->min_wavelength, scene->wavelength_interval, dst_pixels, dst_avgs, dst_vars, 1, seed, &line))
                    fprintf(stderr, "render_image: checkpoint write failed: %s\n", drt_host_checkpoint_error());
                if (!opt->quiet) printf("Adaptive checkpoint after %u rounds, %u pixels active\n", rounds, left);
            }
        }
        if (!rc) done = p.spp;
        if (!rc && !opt->quiet)
            printf("Adaptive: %u rounds, %llu of %llu paths traced (%.1f%%), %u of %llu pixels at %u samples\n", rounds,
                   (unsigned long long)paths, (unsigned long long)p.spp * num_pixels, 100.0 * (f64)paths / ((f64)p.spp * (f64)num_pixels),
                   at_max, (unsigned long long)num_pixels, p.spp);
    }
    else if (!rc && opt && opt->adaptive)
    {
        /* adaptive sampling: rounds until every pixel has converged or holds num_pixel_samples (= max_spp) samples */
        drt_adaptive a;
        memset(&a, 0, sizeof(a));
        a.min_spp = opt->adaptive_min_spp;
        a.max_spp = p.spp;
        a.step = opt->adaptive_step;
        a.rel_error = opt->adaptive_error;
        a.floor = opt->adaptive_floor;
        rc = drt_group_render_adaptive(ctx, &a);
        if (!rc) done = p.spp;
        if (!rc && !opt->quiet)
            printf("Adaptive: %u rounds, %llu of %llu paths traced (%.1f%%), %u of %llu pixels at %u samples\n", a.rounds,
                   (unsigned long long)a.paths, (unsigned long long)p.spp * num_pixels, 100.0 * (f64)a.paths / ((f64)p.spp * (f64)num_pixels),
                   a.pixels_at_max, (unsigned long long)num_pixels, p.spp);
    }
    /* DRT_REGIONS: one sample map over the whole image, num_pixel_samples and inside the regions the largest spp that covers the pixel */
    u32 map_max = 0;
    if (!rc && opt && opt->n_regions)
    {
        u32 *targets = (u32 *)malloc(num_pixels * sizeof(u32));
        if (!targets) rc = -3;
        if (!rc)
        {
            for (u64 px = 0; px < num_pixels; px += 1) targets[px] = p.spp;
            for (u32 k = 0; k < opt->n_regions; k += 1)
            {
                const u32 *r = opt->regions[k];
                const u64 x1 = (u64)r[0] + r[2] < width ? (u64)r[0] + r[2] : width, y1 = (u64)r[1] + r[3] < height ? (u64)r[1] + r[3] : height;
                for (u64 y = r[1]; y < y1; y += 1)
                    for (u64 x = r[0]; x < x1; x += 1)
                        if (targets[y * width + x] < r[4]) targets[y * width + x] = r[4];
            }
            drt_sample_map map;
            memset(&map, 0, sizeof(map));
            map.targets = targets;
            rc = drt_group_render_sample_map(ctx, &map);
            map_max = map.max_count;
            if (!rc) done = map.max_count;
            if (!rc && !opt->quiet)
                printf("Sample map: %u regions, %u rounds, %llu paths traced, %u samples at most\n", opt->n_regions, map.rounds,
                       (unsigned long long)map.paths, map.max_count);
        }
        free(targets);
    }
    u32 step = (opt && opt->checkpoint_spp) ? opt->checkpoint_spp : p.spp;
    while (!rc && done < p.spp)
    {
        u32 n = (p.spp - done < step) ? p.spp - done : step;
        if ((rc = drt_group_render(ctx, done, n))) break;
        done += n;
        if (done < p.spp) /* a checkpoint: the final write below uses the same code */
        {
            if ((rc = drt_group_read_film(ctx, dst_pixels, dst_avgs, dst_vars))) break;
            if (drt_host_write_outputs(config, width, height, S, scene->min_wavelength, scene->wavelength_interval, dst_pixels, dst_avgs, dst_vars, 1, done, seed))
                fprintf(stderr, "render_image: checkpoint write failed: %s\n", drt_host_checkpoint_error());
            if (!(opt && opt->quiet)) printf("Checkpoint at %u / %u samples\n", done, p.spp);
        }
    }
    if (!rc) rc = drt_group_read_film(ctx, dst_pixels, dst_avgs, dst_vars);
    if (!rc) rc = drt_group_get_stats(ctx, &stats);
    /* DRT_DEPTH_CUTS: every cut film through the standard writer (the variance normalised as the standard output's is) under the
     * outputs' names with .depth<d> behind them, and the picture of its sum film by the .spd -> .bmp post-process */
    int cut_bad = 0;
    if (!rc && opt && opt->n_depth_cuts)
    {
        f64 *cut_pixels = (f64 *)malloc(num_pixels * (S + 1) * sizeof(f64));
        f64 *cut_avgs = (f64 *)malloc(num_pixels * S * sizeof(f64)), *cut_vars = (f64 *)malloc(num_pixels * S * sizeof(f64));
        f64 *cmf = (f64 *)malloc((size_t)4 * S * sizeof(f64));
        if (!cut_pixels || !cut_avgs || !cut_vars || !cmf) rc = -3;
        if (!rc)
        {
            const u32 rows[4] = { scene->cmf_rw, scene->cmf_x, scene->cmf_y, scene->cmf_z };
            for (int r = 0; r < 4; r += 1) memcpy(cmf + (size_t)r * S, scene->spds + (size_t)rows[r] * S, (size_t)S * sizeof(f64));
        }
        for (u32 k = 0; !rc && !cut_bad && k < opt->n_depth_cuts; k += 1)
        {
            const u32 d = opt->depth_cuts[k];
            config_arguments cc = *config;
            char bmp[64];
            if ((rc = drt_group_read_depth_film(ctx, k, cut_pixels, cut_avgs, cut_vars))) break;
            if (depth_path(cc.output_spd, config->output_spd, d, ".spd") || depth_path(cc.average_spd, config->average_spd, d, ".spd") ||
                depth_path(cc.variance_spd, config->variance_spd, d, ".spd") || depth_path(bmp, config->output_spd, d, ".bmp") ||
                drt_host_write_outputs(&cc, width, height, S, scene->min_wavelength, scene->wavelength_interval, cut_pixels, cut_avgs, cut_vars, 0, done, seed) ||
                drt_host_spd_file_to_bmp(cc.output_spd, bmp, cmf))
                cut_bad = -1;
            else if (!opt->quiet) printf("Depth cut %u: %s\n", d, cc.output_spd);
        }
        if (cut_bad) fprintf(stderr, "render_image: could not write the outputs of a depth cut\n");
        free(cmf);
        free(cut_vars);
        free(cut_avgs);
        free(cut_pixels);
    }
    /* DRT_SENSOR: the sensor film through the standard writer with n channels for S (the variance normalised as the standard output's
     * is) under the outputs' names with .sensor behind them; with three curves the picture of sum / filter through the identity matrix */
    if (!rc && n_sensor)
    {
        f64 *sn_pixels = (f64 *)malloc(num_pixels * (n_sensor + 1) * sizeof(f64));
        f64 *sn_avgs = (f64 *)malloc(num_pixels * n_sensor * sizeof(f64)), *sn_vars = (f64 *)malloc(num_pixels * n_sensor * sizeof(f64));
        if (!sn_pixels || !sn_avgs || !sn_vars) rc = -3;
        if (!rc) rc = drt_group_read_sensor_film(ctx, sn_pixels, sn_avgs, sn_vars);
        if (!rc)
        {
            config_arguments cc = *config;
            char bmp[64];
            if (sensor_path(cc.output_spd, config->output_spd, ".spd") || sensor_path(cc.average_spd, config->average_spd, ".spd") ||
                sensor_path(cc.variance_spd, config->variance_spd, ".spd") || sensor_path(bmp, config->output_spd, ".bmp") ||
                drt_host_write_outputs(&cc, width, height, n_sensor, scene->min_wavelength, scene->wavelength_interval, sn_pixels, sn_avgs, sn_vars, 0, done, seed))
                cut_bad = -1;
            else if (n_sensor == 3)
            {
                /* drt_read_sensor_bgra's rule with the identity matrix: 1 * v, then + 0 * v for the other two, in order */
                u8 *fb = (u8 *)malloc(num_pixels * 4);
                if (!fb) cut_bad = -1;
                for (u64 i = 0; fb && i < num_pixels; i += 1)
                    for (int r = 0; r < 3; r += 1)
                    {
                        f64 f = 0.0;
                        for (int k = 0; k < 3; k += 1)
                        {
                            const f64 t = (k == r ? 1.0 : 0.0) * (sn_pixels[i * 4 + k] / sn_pixels[i * 4 + 3]);
                            f = k == 0 ? t : f + t;
                        }
                        f = (f < 0.0) ? 0.0 : f;
                        f = (f > 1.0) ? 1.0 : f;
                        fb[i * 4 + 2 - r] = (f == f) ? (u8)(f * 255.0) : (u8)0;
                        fb[i * 4 + 3] = 255;
                    }
                if (fb && drt_host_write_bmp_bgra(bmp, width, height, fb) != 0) cut_bad = -1;
                free(fb);
            }
            if (cut_bad) fprintf(stderr, "render_image: could not write the outputs of the sensor film\n");
            else if (!opt->quiet) printf("Sensor film: %u channels, %s\n", n_sensor, cc.output_spd);
        }
        free(sn_vars);
        free(sn_avgs);
        free(sn_pixels);
    }
    free(sensor_curves);
    /* DRT_BUCKETS: every bucket film through the standard writer (the variance normalised as the standard output's is) under the outputs'
     * names with .bucket<b> behind them; with two buckets or more the resolve: estimate and error under the average file's header, and
     * the estimate's picture by the .spd -> .bmp post-process */
    if (!rc && opt && opt->n_buckets)
    {
        const u32 n_buckets = opt->n_buckets;
        f64 *bk_pixels = (f64 *)malloc(num_pixels * (S + 1) * sizeof(f64));
        f64 *bk_avgs = (f64 *)malloc(num_pixels * S * sizeof(f64)), *bk_vars = (f64 *)malloc(num_pixels * S * sizeof(f64));
        f64 *cmf = (f64 *)malloc((size_t)4 * S * sizeof(f64));
        if (!bk_pixels || !bk_avgs || !bk_vars || !cmf) rc = -3;
        if (!rc)
        {
            const u32 rows[4] = { scene->cmf_rw, scene->cmf_x, scene->cmf_y, scene->cmf_z };
            for (int r = 0; r < 4; r += 1) memcpy(cmf + (size_t)r * S, scene->spds + (size_t)rows[r] * S, (size_t)S * sizeof(f64));
        }
        for (u32 b = 0; !rc && !cut_bad && b < n_buckets; b += 1)
        {
            config_arguments cc = *config;
            if ((rc = drt_group_read_bucket_film(ctx, b, bk_pixels, bk_avgs, bk_vars))) break;
            /* the filter column says how many of the samples fell into this bucket */
            if (bucket_path(cc.output_spd, config->output_spd, b, ".spd") || bucket_path(cc.average_spd, config->average_spd, b, ".spd") ||
                bucket_path(cc.variance_spd, config->variance_spd, b, ".spd") ||
                drt_host_write_outputs(&cc, width, height, S, scene->min_wavelength, scene->wavelength_interval, bk_pixels, bk_avgs, bk_vars, 0,
                                       (done - b + n_buckets - 1) / n_buckets, seed))
                cut_bad = -1;
        }
        if (!rc && !cut_bad && n_buckets >= 2)
        {
            char est[64], err[64], bmp[64];
            if (!(rc = drt_group_resolve_buckets(ctx, opt->bucket_trim)) && !(rc = drt_group_read_bucket_resolve(ctx, bk_avgs, bk_vars)))
            {
                if (robust_path(est, config->average_spd, ".spd") || robust_path(err, config->variance_spd, ".spd") || robust_path(bmp, config->output_spd, ".bmp") ||
                    publish_spd(est, width, height, S, scene->min_wavelength, scene->wavelength_interval, bk_avgs) ||
                    publish_spd(err, width, height, S, scene->min_wavelength, scene->wavelength_interval, bk_vars) || drt_host_spd_file_to_bmp(est, bmp, cmf))
                    cut_bad = -1;
            }
        }
        if (cut_bad) fprintf(stderr, "render_image: could not write the outputs of the bucket films\n");
        else if (!rc && !opt->quiet) printf("Bucket films: %u buckets, trim %u\n", n_buckets, opt->bucket_trim);
        free(cmf);
        free(bk_vars);
        free(bk_avgs);
        free(bk_pixels);
    }
    /* DRT_LOBES: every lobe film through the standard writer (the variance normalised as the standard output's is) under the outputs'
     * names with .lobe<k> behind them, the picture of its mean by the .spd -> .bmp post-process, and the list of the films' names */
    if (!rc && opt && opt->n_lobes)
    {
        const u32 n_lobes = opt->n_lobes;
        f64 *lb_pixels = (f64 *)malloc(num_pixels * (S + 1) * sizeof(f64));
        f64 *lb_avgs = (f64 *)malloc(num_pixels * S * sizeof(f64)), *lb_vars = (f64 *)malloc(num_pixels * S * sizeof(f64));
        f64 *cmf = (f64 *)malloc((size_t)4 * S * sizeof(f64));
        if (!lb_pixels || !lb_avgs || !lb_vars || !cmf) rc = -3;
        if (!rc)
        {
            const u32 rows[4] = { scene->cmf_rw, scene->cmf_x, scene->cmf_y, scene->cmf_z };
            for (int r = 0; r < 4; r += 1) memcpy(cmf + (size_t)r * S, scene->spds + (size_t)rows[r] * S, (size_t)S * sizeof(f64));
        }
        for (u32 k = 0; !rc && !cut_bad && k < n_lobes; k += 1)
        {
            config_arguments cc = *config;
            char bmp[64];
            if ((rc = drt_group_read_lobe_film(ctx, k, lb_pixels, lb_avgs, lb_vars))) break;
            if (lobe_path(cc.output_spd, config->output_spd, k, ".spd") || lobe_path(cc.average_spd, config->average_spd, k, ".spd") ||
                lobe_path(cc.variance_spd, config->variance_spd, k, ".spd") || lobe_path(bmp, config->output_spd, k, ".bmp") ||
                drt_host_write_outputs(&cc, width, height, S, scene->min_wavelength, scene->wavelength_interval, lb_pixels, lb_avgs, lb_vars, 0, done, seed) ||
                drt_host_spd_file_to_bmp(cc.average_spd, bmp, cmf))
                cut_bad = -1;
        }
        if (!rc && !cut_bad)
        {
            char txt[64];
            FILE *f = lobes_txt_path(txt, config->output_spd) ? NULL : fopen(txt, "w");
            if (!f) cut_bad = -1;
            else
            {
                for (u32 k = 0; k < n_lobes; k += 1) fprintf(f, "%u %s\n", k, opt->lobe_names[k]);
                if (fclose(f)) cut_bad = -1;
            }
        }
        if (cut_bad) fprintf(stderr, "render_image: could not write the outputs of the lobe films\n");
        else if (!rc && !opt->quiet) printf("Lobe films: %u films\n", n_lobes);
        free(cmf);
        free(lb_vars);
        free(lb_avgs);
        free(lb_pixels);
    }
    /* the denoised film, while the devices still hold the scene's tables (the film itself is not changed) */
    f64 *dn_mean = NULL, *dn_var = NULL;
    if (!rc && opt && opt->denoise)
    {
        drt_denoise dn;
        memset(&dn, 0, sizeof(dn));
        dn.radius = opt->denoise_radius;
        dn.patch = opt->denoise_patch;
        dn.k = opt->denoise_k;
        dn.alpha = opt->denoise_alpha;
        dn_mean = (f64 *)malloc(num_pixels * S * sizeof(f64));
        dn_var = (f64 *)malloc(num_pixels * S * sizeof(f64));
        if (!dn_mean || !dn_var) rc = -3;
        if (!rc) rc = drt_group_denoise(ctx, &dn, dn_mean, dn_var);
        if (!rc && !opt->quiet)
            printf("Denoised: radius %u, patch %u, k %g, alpha %g: %.3f ms on the device, %u pixels passed through\n", dn.radius, dn.patch, dn.k,
                   dn.alpha, dn.kernel_ms, dn.unusable);
    }
    /* the first-hit feature buffers of the finished film, every pixel at the count it holds (the film itself is not changed) */
    f64 *ft_mean = NULL, *ft_m2 = NULL;
    if (!rc && opt && opt->features)
    {
        drt_features ft;
        memset(&ft, 0, sizeof(ft));
        ft_mean = (f64 *)malloc(num_pixels * DRT_FEATURE_CHANNELS * sizeof(f64));
        ft_m2 = (f64 *)malloc(num_pixels * DRT_FEATURE_CHANNELS * sizeof(f64));
        if (!ft_mean || !ft_m2) rc = -3;
        if (!rc) rc = drt_group_render_features(ctx, &ft, ft_mean, ft_m2, NULL);
        if (!rc && !opt->quiet)
            printf("Features: %llu camera rays, %.3f ms on the device, %u pixels see nothing\n", (unsigned long long)ft.rays, ft.kernel_ms, ft.empty_pixels);
    }
    /* the ID mattes of the finished film, likewise */
    int32_t *mt_ids = NULL;
    u32 *mt_counts = NULL, *mt_tail = NULL;
    if (!rc && opt && opt->mattes)
    {
        drt_mattes mt;
        memset(&mt, 0, sizeof(mt));
        mt_ids = (int32_t *)malloc(num_pixels * MATTE_CHANNELS * sizeof(int32_t));
        mt_counts = (u32 *)malloc(num_pixels * MATTE_CHANNELS * sizeof(u32));
        mt_tail = (u32 *)malloc(num_pixels * 4 * sizeof(u32));
        if (!mt_ids || !mt_counts || !mt_tail) rc = -3;
        if (!rc) rc = drt_group_render_mattes(ctx, &mt, mt_ids, mt_counts, mt_tail);
        if (!rc && !opt->quiet)
            printf("Mattes: %llu camera rays, %.3f ms on the device, %u pixels see nothing, %u / %u see more than %d surfaces / materials\n",
                   (unsigned long long)mt.rays, mt.kernel_ms, mt.empty_pixels, mt.overflow_pixels[0], mt.overflow_pixels[1], DRT_MATTE_SLOTS);
    }
    /* DRT_PICK: the closest hit of each entry's camera ray (nothing on the devices changes) */
    drt_ray_hit pick_hits[DRT_HOST_MAX_PICKS];
    u32 n_picks = (opt && !rc) ? opt->n_picks : 0;
    if (n_picks) rc = drt_group_cast_pixels(ctx, &opt->pick_xy[0][0], opt->pick_sample, n_picks, NULL, NULL, pick_hits);
    if (rc) n_picks = 0;
    /* the .bmp pixels come from the film while it is still on the device (drt_read_bgra: the same bytes as converting the
     * .spd files on the host, host/drt_bmp.c, without reading 1.7 GB back from disk) */
    u8 *bgra[3] = { NULL, NULL, NULL };
    const char *bmp_path[3] = { config->output_bmp, config->average_bmp, config->variance_bmp };
    for (int k = 0; !rc && k < 3 && config->output_bmp[0]; k += 1)
    {
        if (!bmp_path[k][0]) continue;
        bgra[k] = (u8 *)malloc(num_pixels * 4 + 4);
        if (!bgra[k]) { rc = -3; break; }
        rc = drt_group_read_bgra(ctx, k, bgra[k]);
    }
    drt_group_destroy(ctx);
    f64 t1 = now_ms();
    if (rc != 0)
    {
        fprintf(stderr, "render_image: the HIP launcher failed (%d): %s\n", rc, drt_last_error());
        for (int k = 0; k < 3; k += 1) free(bgra[k]);
        free(mt_tail);
        free(mt_counts);
        free(mt_ids);
        free(ft_m2);
        free(ft_mean);
        free(dn_var);
        free(dn_mean);
        free(dst_vars);
        free(dst_avgs);
        free(dst_pixels);
        drt_host_free_scene(hs);
        return rc;
    }
    if (!(opt && opt->quiet))
    {
        /* the reference's report, src/daily_ray_trace.c:753-756; a "sample" is one sample pass over the image at the rate of one
         * kernel pair (drt_stats, include/drt_hip.h) */
        printf("Min sample time: %fms\n", stats.min_sample_ms);
        printf("Max sample time: %fms\n", stats.max_sample_ms);
        printf("Avg sample time: %fms\n", stats.avg_sample_ms);
        printf("Total render time: %fms (device %fms: trace %fms, shade+film %fms, %u kernel pairs)\n", t1 - t0, stats.total_ms,
               stats.trace_ms, stats.shade_ms, stats.launches);
        printf("Paths: %llu  closest-hit scans/path: %.3f  shaded vertices/path: %.3f  Mpaths/s (device): %.2f\n",
               (unsigned long long)stats.paths, (f64)stats.closest_hit_scans / (f64)stats.paths,
               (f64)stats.shaded_vertices / (f64)stats.paths, (f64)stats.paths / (stats.total_ms * 1e3));
    }

    for (u32 k = 0; k < n_picks; k += 1)
    {
        const drt_ray_hit *h = &pick_hits[k];
        if (h->index < 0) printf("pick %u %u %u miss\n", opt->pick_xy[k][0], opt->pick_xy[k][1], opt->pick_sample[k]);
        else
            printf("pick %u %u %u surface %d %s material %u %s distance %.17g position %.17g %.17g %.17g\n", opt->pick_xy[k][0], opt->pick_xy[k][1],
                   opt->pick_sample[k], h->index, drt_host_surface_name(hs, (u32)h->index), h->surface_material,
                   drt_host_material_name(hs, h->surface_material), h->distance, h->position[0], h->position[1], h->position[2]);
    }

    int wrc;
    if (opt && opt->adaptive && opt->adaptive_checkpoint_rounds)
    {
        const drt_host_adaptive_line line = { opt->adaptive_min_spp, p.spp, opt->adaptive_step, opt->adaptive_error, opt->adaptive_floor };
        wrc = drt_host_write_outputs_adaptive(config, width, height, S, scene->min_wavelength, scene->wavelength_interval, dst_pixels, dst_avgs, dst_vars, 1, seed, &line);
    }
    else
        wrc = drt_host_write_outputs(config, width, height, S, scene->min_wavelength, scene->wavelength_interval, dst_pixels, dst_avgs, dst_vars,
                                     (opt && opt->checkpoint_spp) ? 1 : 0, done, seed);
    if (wrc) fprintf(stderr, "render_image: %s\n", drt_host_checkpoint_error());
    int w0 = wrc, w1 = 0, w2 = 0;
    if (!w0 && dn_mean)
    {
        /* both under the average file's header (no filter column), each by temporary name + rename */
        w1 = publish_spd(opt->denoise_spd, width, height, S, scene->min_wavelength, scene->wavelength_interval, dn_mean);
        if (!w1) w2 = publish_spd(opt->denoise_var_spd, width, height, S, scene->min_wavelength, scene->wavelength_interval, dn_var);
        if (w1 || w2) fprintf(stderr, "render_image: could not write the denoised .spd outputs\n");
    }
    int w3 = 0;
    if (!(w0 || w1 || w2) && ft_mean)
    {
        /* mean and m2 as 8-"wavelength" files without a filter column, then the three pictures of the mean; depth from its smallest
         * to its largest value over the pixels that see anything */
        static const char *const suffix[3] = { "normal", "depth", "coverage" };
        w3 = publish_spd(opt->features_spd, width, height, DRT_FEATURE_CHANNELS, scene->min_wavelength, scene->wavelength_interval, ft_mean);
        if (!w3) w3 = publish_spd(opt->features_m2_spd, width, height, DRT_FEATURE_CHANNELS, scene->min_wavelength, scene->wavelength_interval, ft_m2);
        f64 zlo = 0.0, zhi = 0.0;
        int seen = 0;
        for (u64 px = 0; px < num_pixels; px += 1)
        {
            const f64 *m = ft_mean + px * DRT_FEATURE_CHANNELS;
            if (!(m[4] > 0.0)) continue;
            if (!seen || m[3] < zlo) zlo = m[3];
            if (!seen || m[3] > zhi) zhi = m[3];
            seen = 1;
        }
        if (!seen || !(zhi > zlo) || !isfinite(zlo) || !isfinite(zhi)) { zlo = 0.0; zhi = 1.0; }
        u8 *fb = (u8 *)malloc(num_pixels * 4 + 4);
        if (!fb) w3 = -1;
        for (int k = 0; !w3 && k < 3; k += 1)
        {
            char path[300], tmp[304];
            if (snprintf(path, sizeof(path), "%s.%s.bmp", config->output_spd, suffix[k]) >= (int)sizeof(path)) { w3 = -1; break; }
            snprintf(tmp, sizeof(tmp), "%s.tmp", path);
            drt_host_feature_bgra(ft_mean, num_pixels, k, k == 0 ? -1.0 : k == 1 ? zlo : 0.0, k == 1 ? zhi : 1.0, fb);
            if (drt_host_write_bmp_bgra(tmp, width, height, fb) != 0 || rename(tmp, path) != 0) w3 = -1;
        }
        free(fb);
        if (w3) fprintf(stderr, "render_image: could not write the feature outputs\n");
    }
    int w4 = 0;
    if (!(w0 || w1 || w2 || w3) && mt_ids)
    {
        w4 = publish_mattes(config->output_spd, hs, width, height, mt_ids, mt_counts, mt_tail);
        if (w4) fprintf(stderr, "render_image: could not write the matte outputs\n");
    }
    int w5 = 0;
    if (!(w0 || w1 || w2 || w3 || w4) && opt && opt->n_regions)
    {
        /* DRT_REGIONS: every pixel's count (its filter sum) over the largest, grey */
        char path[80], tmp[84];
        u8 *fb = (u8 *)malloc(num_pixels * 4 + 4);
        snprintf(path, sizeof(path), "%s.counts.bmp", config->output_spd);
        snprintf(tmp, sizeof(tmp), "%s.tmp", path);
        if (!fb) w5 = -1;
        for (u64 px = 0; !w5 && px < num_pixels; px += 1)
        {
            const u8 v = (u8)(255.0 * dst_pixels[px * (S + 1) + S] / (f64)map_max + 0.5);
            fb[px * 4 + 0] = fb[px * 4 + 1] = fb[px * 4 + 2] = v;
            fb[px * 4 + 3] = 255;
        }
        if (!w5 && (drt_host_write_bmp_bgra(tmp, width, height, fb) != 0 || rename(tmp, path) != 0)) w5 = -1;
        free(fb);
        if (w5) fprintf(stderr, "render_image: could not write the picture of the sample counts\n");
    }
    /* post-process like the reference's main(): each film -> linear RGB -> BMP (src/win32_main.c:150-152) */
    if (!(w0 || w1 || w2 || w3 || w4 || w5))
    {
        int bad = 0;
        for (int k = 0; k < 3; k += 1)
            if (bgra[k]) bad |= drt_host_write_bmp_bgra(bmp_path[k], width, height, bgra[k]);
        if (bad) fprintf(stderr, "render_image: could not write one of the .bmp outputs\n");
    }
    for (int k = 0; k < 3; k += 1) free(bgra[k]);
    free(mt_tail);
    free(mt_counts);
    free(mt_ids);
    free(ft_m2);
    free(ft_mean);
    free(dn_var);
    free(dn_mean);
    if (stats_out) *stats_out = stats;
    free(dst_vars);
    free(dst_avgs);
    free(dst_pixels);
    drt_host_free_scene(hs);
    return (w0 || w1 || w2 || w3 || w4 || w5 || cut_bad) ? -2 : 0;
}

/* a whole-string number from the environment: 0 and *out set, -1 (and a message naming the variable) when it does not parse */
static int env_double(const char *name, double *out)
{
    const char *e = getenv(name);
    char *end = NULL;
    errno = 0;
    double v = strtod(e, &end);
    if (!*e || *end || errno) { fprintf(stderr, "render_image: %s=\"%s\" is not a number\n", name, e); return -1; }
    *out = v;
    return 0;
}

static int env_u32(const char *name, u32 *out)
{
    const char *e = getenv(name);
    char *end = NULL;
    errno = 0;
    unsigned long long v = strtoull(e, &end, 10);
    if (!*e || *end || errno || e[0] == '-' || v > 0xFFFFFFFFull) { fprintf(stderr, "render_image: %s=\"%s\" is not a whole number\n", name, e); return -1; }
    *out = (u32)v;
    return 0;
}

/* DRT_ADAPTIVE_*: parsed and checked here, before any device call. DRT_ADAPTIVE_ERROR=<rel_error> turns adaptive sampling on;
 * DRT_ADAPTIVE_MIN_SPP (default min(16, num_pixel_samples)), DRT_ADAPTIVE_STEP (default min_spp), DRT_ADAPTIVE_FLOOR (default 0);
 * DRT_ADAPTIVE_CHECKPOINT_ROUNDS=k (a whole number, 1 or more) writes a checkpoint after every k rendering rounds, DRT_ADAPTIVE_RESUME=1
 * continues from one. */
static int adaptive_options(const config_arguments *config, drt_host_options *opt)
{
    static const char *const names[] = { "DRT_ADAPTIVE_MIN_SPP", "DRT_ADAPTIVE_STEP", "DRT_ADAPTIVE_FLOOR", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS", "DRT_ADAPTIVE_RESUME" };
    if (!getenv("DRT_ADAPTIVE_ERROR"))
    {
        for (int k = 0; k < 5; k += 1)
            if (getenv(names[k])) { fprintf(stderr, "render_image: %s is set but DRT_ADAPTIVE_ERROR is not\n", names[k]); return -1; }
        return 0;
    }
    const u32 max_spp = config->num_pixel_samples;
    opt->adaptive = 1;
    if (env_double("DRT_ADAPTIVE_ERROR", &opt->adaptive_error)) return -1;
    if (!isfinite(opt->adaptive_error) || !(opt->adaptive_error > 0.0))
    { fprintf(stderr, "render_image: DRT_ADAPTIVE_ERROR=%s: a finite number above 0\n", getenv("DRT_ADAPTIVE_ERROR")); return -1; }
    opt->adaptive_min_spp = max_spp < 16 ? max_spp : 16;
    if (getenv("DRT_ADAPTIVE_MIN_SPP") && env_u32("DRT_ADAPTIVE_MIN_SPP", &opt->adaptive_min_spp)) return -1;
    if (opt->adaptive_min_spp < 2 || opt->adaptive_min_spp > max_spp)
    {
        fprintf(stderr, "render_image: DRT_ADAPTIVE_MIN_SPP=%u: from 2 to num_pixel_samples (%u)\n", opt->adaptive_min_spp, max_spp);
        return -1;
    }
    opt->adaptive_step = opt->adaptive_min_spp;
    if (getenv("DRT_ADAPTIVE_STEP") && env_u32("DRT_ADAPTIVE_STEP", &opt->adaptive_step)) return -1;
    if (opt->adaptive_step < 1) { fprintf(stderr, "render_image: DRT_ADAPTIVE_STEP=%u: at least 1\n", opt->adaptive_step); return -1; }
    opt->adaptive_floor = 0.0;
    if (getenv("DRT_ADAPTIVE_FLOOR") && env_double("DRT_ADAPTIVE_FLOOR", &opt->adaptive_floor)) return -1;
    if (!isfinite(opt->adaptive_floor) || !(opt->adaptive_floor >= 0.0))
    { fprintf(stderr, "render_image: DRT_ADAPTIVE_FLOOR=%s: a finite number, 0 or more\n", getenv("DRT_ADAPTIVE_FLOOR")); return -1; }
    if (getenv("DRT_ADAPTIVE_CHECKPOINT_ROUNDS"))
    {
        if (env_u32("DRT_ADAPTIVE_CHECKPOINT_ROUNDS", &opt->adaptive_checkpoint_rounds)) return -1;
        if (opt->adaptive_checkpoint_rounds < 1) { fprintf(stderr, "render_image: DRT_ADAPTIVE_CHECKPOINT_ROUNDS=0: at least 1\n"); return -1; }
    }
    if (getenv("DRT_ADAPTIVE_RESUME") && env_u32("DRT_ADAPTIVE_RESUME", &opt->adaptive_resume)) return -1;
    if (getenv("DRT_CHECKPOINT_SPP")) { fprintf(stderr, "render_image: DRT_ADAPTIVE_ERROR cannot be combined with DRT_CHECKPOINT_SPP\n"); return -1; }
    if (getenv("DRT_RESUME")) { fprintf(stderr, "render_image: DRT_ADAPTIVE_ERROR cannot be combined with DRT_RESUME\n"); return -1; }
    return 0;
}

/* DRT_DENOISE_*: parsed and checked here, before any device call. DRT_DENOISE_K=<k> turns the denoiser on; DRT_DENOISE_RADIUS (default 5),
 * DRT_DENOISE_PATCH (1), DRT_DENOISE_ALPHA (1); the outputs go to DRT_DENOISE_SPD (default <output_spd>.denoised.spd) and
 * DRT_DENOISE_VAR_SPD (default <variance_spd>.denoised.spd). */
static int denoise_options(const config_arguments *config, drt_host_options *opt)
{
    static const char *const names[] = { "DRT_DENOISE_RADIUS", "DRT_DENOISE_PATCH", "DRT_DENOISE_ALPHA", "DRT_DENOISE_SPD", "DRT_DENOISE_VAR_SPD" };
    if (!getenv("DRT_DENOISE_K"))
    {
        for (int k = 0; k < 5; k += 1)
            if (getenv(names[k])) { fprintf(stderr, "render_image: %s is set but DRT_DENOISE_K is not\n", names[k]); return -1; }
        return 0;
    }
    opt->denoise = 1;
    if (env_double("DRT_DENOISE_K", &opt->denoise_k)) return -1;
    if (!isfinite(opt->denoise_k) || !(opt->denoise_k > 0.0))
    { fprintf(stderr, "render_image: DRT_DENOISE_K=%s: a finite number above 0\n", getenv("DRT_DENOISE_K")); return -1; }
    opt->denoise_radius = 5;
    if (getenv("DRT_DENOISE_RADIUS") && env_u32("DRT_DENOISE_RADIUS", &opt->denoise_radius)) return -1;
    if (opt->denoise_radius > 10) { fprintf(stderr, "render_image: DRT_DENOISE_RADIUS=%u: from 0 to 10\n", opt->denoise_radius); return -1; }
    opt->denoise_patch = 1;
    if (getenv("DRT_DENOISE_PATCH") && env_u32("DRT_DENOISE_PATCH", &opt->denoise_patch)) return -1;
    if (opt->denoise_patch > 3) { fprintf(stderr, "render_image: DRT_DENOISE_PATCH=%u: from 0 to 3\n", opt->denoise_patch); return -1; }
    opt->denoise_alpha = 1.0;
    if (getenv("DRT_DENOISE_ALPHA") && env_double("DRT_DENOISE_ALPHA", &opt->denoise_alpha)) return -1;
    if (!isfinite(opt->denoise_alpha) || !(opt->denoise_alpha >= 0.0))
    { fprintf(stderr, "render_image: DRT_DENOISE_ALPHA=%s: a finite number, 0 or more\n", getenv("DRT_DENOISE_ALPHA")); return -1; }
    const char *e = getenv("DRT_DENOISE_SPD");
    int n = e ? snprintf(opt->denoise_spd, sizeof(opt->denoise_spd), "%s", e)
              : snprintf(opt->denoise_spd, sizeof(opt->denoise_spd), "%s.denoised.spd", config->output_spd);
    if (n <= 0 || n >= (int)sizeof(opt->denoise_spd)) { fprintf(stderr, "render_image: DRT_DENOISE_SPD: a path of 1 to %d characters\n", (int)sizeof(opt->denoise_spd) - 1); return -1; }
    e = getenv("DRT_DENOISE_VAR_SPD");
    n = e ? snprintf(opt->denoise_var_spd, sizeof(opt->denoise_var_spd), "%s", e)
          : snprintf(opt->denoise_var_spd, sizeof(opt->denoise_var_spd), "%s.denoised.spd", config->variance_spd);
    if (n <= 0 || n >= (int)sizeof(opt->denoise_var_spd)) { fprintf(stderr, "render_image: DRT_DENOISE_VAR_SPD: a path of 1 to %d characters\n", (int)sizeof(opt->denoise_var_spd) - 1); return -1; }
    if (strcmp(opt->denoise_spd, opt->denoise_var_spd) == 0) { fprintf(stderr, "render_image: DRT_DENOISE_SPD and DRT_DENOISE_VAR_SPD name the same file\n"); return -1; }
    return 0;
}

/* DRT_FEATURES*: parsed and checked here, before any device call. DRT_FEATURES=1 turns the first-hit feature buffers on (0: off, anything
 * else is refused); the two .spd outputs go to DRT_FEATURES_SPD (default <output_spd>.features.spd) and DRT_FEATURES_M2_SPD (default
 * <variance_spd>.features.spd). */
static int features_options(const config_arguments *config, drt_host_options *opt)
{
    static const char *const names[] = { "DRT_FEATURES_SPD", "DRT_FEATURES_M2_SPD" };
    const char *e = getenv("DRT_FEATURES");
    if (e && strcmp(e, "0") != 0 && strcmp(e, "1") != 0) { fprintf(stderr, "render_image: DRT_FEATURES=\"%s\": 0 or 1\n", e); return -1; }
    if (!e || e[0] == '0')
    {
        for (int k = 0; k < 2; k += 1)
            if (getenv(names[k])) { fprintf(stderr, "render_image: %s is set but DRT_FEATURES is not 1\n", names[k]); return -1; }
        return 0;
    }
    opt->features = 1;
    e = getenv("DRT_FEATURES_SPD");
    int n = e ? snprintf(opt->features_spd, sizeof(opt->features_spd), "%s", e)
              : snprintf(opt->features_spd, sizeof(opt->features_spd), "%s.features.spd", config->output_spd);
    if (n <= 0 || n >= (int)sizeof(opt->features_spd)) { fprintf(stderr, "render_image: DRT_FEATURES_SPD: a path of 1 to %d characters\n", (int)sizeof(opt->features_spd) - 1); return -1; }
    e = getenv("DRT_FEATURES_M2_SPD");
    n = e ? snprintf(opt->features_m2_spd, sizeof(opt->features_m2_spd), "%s", e)
          : snprintf(opt->features_m2_spd, sizeof(opt->features_m2_spd), "%s.features.spd", config->variance_spd);
    if (n <= 0 || n >= (int)sizeof(opt->features_m2_spd)) { fprintf(stderr, "render_image: DRT_FEATURES_M2_SPD: a path of 1 to %d characters\n", (int)sizeof(opt->features_m2_spd) - 1); return -1; }
    if (strcmp(opt->features_spd, opt->features_m2_spd) == 0) { fprintf(stderr, "render_image: DRT_FEATURES_SPD and DRT_FEATURES_M2_SPD name the same file\n"); return -1; }
    return 0;
}

/* DRT_MATTES: parsed and checked here, before any device call. 1 turns the ID mattes on, 0 is off, anything else is refused. (The
 * program renders the spectral film only, so the counts the mattes need are always there.) */
static int mattes_options(drt_host_options *opt)
{
    const char *e = getenv("DRT_MATTES");
    if (e && strcmp(e, "0") != 0 && strcmp(e, "1") != 0) { fprintf(stderr, "render_image: DRT_MATTES=\"%s\": 0 or 1\n", e); return -1; }
    opt->mattes = e && e[0] == '1';
    return 0;
}

/* DRT_PICK="x,y[,sample][;x,y[,sample]...]": parsed and checked here, before any device call. Whole decimal numbers, the sample 0 when
 * left out, DRT_HOST_MAX_PICKS entries at most, every pixel inside the output_width x output_height image. */
static int pick_number(const char **c, u32 *out)
{
    if (**c < '0' || **c > '9') return -1;
    char *end;
    errno = 0;
    unsigned long long v = strtoull(*c, &end, 10);
    if (errno || v > 0xFFFFFFFFull) return -1;
    *out = (u32)v;
    *c = end;
    return 0;
}

static int pick_options(const config_arguments *config, drt_host_options *opt)
{
    const char *e = getenv("DRT_PICK");
    opt->n_picks = 0;
    if (!e) return 0;
    const char *c = e;
    for (;;)
    {
        u32 x, y, sample = 0;
        if (opt->n_picks == DRT_HOST_MAX_PICKS) { fprintf(stderr, "render_image: DRT_PICK: %d entries at most\n", DRT_HOST_MAX_PICKS); return -1; }
        if (pick_number(&c, &x) || *c != ',') break;
        c += 1;
        if (pick_number(&c, &y)) break;
        if (*c == ',')
        {
            c += 1;
            if (pick_number(&c, &sample)) break;
        }
        if (x >= (u32)config->output_width || y >= (u32)config->output_height)
        {
            fprintf(stderr, "render_image: DRT_PICK: pixel (%u, %u) is outside the %u x %u image\n", x, y, (u32)config->output_width, (u32)config->output_height);
            return -1;
        }
        opt->pick_xy[opt->n_picks][0] = x;
        opt->pick_xy[opt->n_picks][1] = y;
        opt->pick_sample[opt->n_picks] = sample;
        opt->n_picks += 1;
        if (*c == 0) return 0;
        if (*c != ';') break;
        c += 1;
    }
    fprintf(stderr, "render_image: DRT_PICK=\"%s\": x,y[,sample] entries of whole numbers, separated by ';' (stopped at character %d)\n", e, (int)(c - e));
    return -1;
}

/* DRT_PROJECTION=equirect | ortho (with DRT_ORTHO_WIDTH=<w>, the rectangle's width in scene units): parsed and checked here, before any
 * device call, after the options it cannot be combined with. */
static int projection_options(drt_host_options *opt)
{
    const char *e = getenv("DRT_PROJECTION"), *w = getenv("DRT_ORTHO_WIDTH");
    opt->projection = 0;
    if (!e)
    {
        if (w) { fprintf(stderr, "render_image: DRT_ORTHO_WIDTH is set but DRT_PROJECTION is not ortho\n"); return -1; }
        return 0;
    }
    if (strcmp(e, "equirect") == 0) opt->projection = DRT_HOST_PROJECTION_EQUIRECT;
    else if (strcmp(e, "ortho") == 0) opt->projection = DRT_HOST_PROJECTION_ORTHO;
    else { fprintf(stderr, "render_image: DRT_PROJECTION=\"%s\": equirect or ortho\n", e); return -1; }
    if (opt->projection == DRT_HOST_PROJECTION_ORTHO)
    {
        if (!w) { fprintf(stderr, "render_image: DRT_PROJECTION=ortho needs DRT_ORTHO_WIDTH\n"); return -1; }
        if (env_double("DRT_ORTHO_WIDTH", &opt->ortho_width)) return -1;
        if (!isfinite(opt->ortho_width) || !(opt->ortho_width > 0.0))
        { fprintf(stderr, "render_image: DRT_ORTHO_WIDTH=%s: a finite number above 0\n", w); return -1; }
    }
    else if (w) { fprintf(stderr, "render_image: DRT_ORTHO_WIDTH is set but DRT_PROJECTION is not ortho\n"); return -1; }
    if (opt->features) { fprintf(stderr, "render_image: DRT_PROJECTION cannot be combined with DRT_FEATURES, which asks for the camera's rays\n"); return -1; }
    if (opt->mattes) { fprintf(stderr, "render_image: DRT_PROJECTION cannot be combined with DRT_MATTES, which asks for the camera's rays\n"); return -1; }
    if (opt->n_picks) { fprintf(stderr, "render_image: DRT_PROJECTION cannot be combined with DRT_PICK, which asks for the camera's rays\n"); return -1; }
    return 0;
}

/* DRT_TURNTABLE=n (a whole number, 1 or more): parsed and checked here, before any device call, after the options it cannot be combined with. */
static int turntable_options(drt_host_options *opt)
{
    opt->turntable = 0;
    if (!getenv("DRT_TURNTABLE")) return 0;
    if (env_u32("DRT_TURNTABLE", &opt->turntable)) return -1;
    if (opt->turntable < 1 || opt->turntable > 9999) { fprintf(stderr, "render_image: DRT_TURNTABLE=%u: from 1 to 9999 frames\n", opt->turntable); return -1; }
    static const char *const names[] = { "DRT_CHECKPOINT_SPP", "DRT_RESUME", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS", "DRT_ADAPTIVE_RESUME", "DRT_PROJECTION",
                                         "DRT_DENOISE_K", "DRT_PICK" };
    for (int k = 0; k < 7; k += 1)
        if (getenv(names[k])) { fprintf(stderr, "render_image: DRT_TURNTABLE cannot be combined with %s\n", names[k]); return -1; }
    if (opt->features) { fprintf(stderr, "render_image: DRT_TURNTABLE cannot be combined with DRT_FEATURES\n"); return -1; }
    if (opt->mattes) { fprintf(stderr, "render_image: DRT_TURNTABLE cannot be combined with DRT_MATTES\n"); return -1; }
    return 0;
}

/* DRT_LIGHT_LEVELS="k0,k1,..." (finite numbers, DRT_HOST_MAX_LEVELS at most): parsed and checked here, before any device call, after the
 * options it cannot be combined with. */
static int light_levels_options(drt_host_options *opt)
{
    opt->n_levels = 0;
    const char *e = getenv("DRT_LIGHT_LEVELS");
    if (!e) return 0;
    static const char *const names[] = { "DRT_TURNTABLE", "DRT_CHECKPOINT_SPP", "DRT_RESUME", "DRT_ADAPTIVE_CHECKPOINT_ROUNDS", "DRT_ADAPTIVE_RESUME",
                                         "DRT_PROJECTION", "DRT_DENOISE_K", "DRT_PICK" };
    for (int k = 0; k < 8; k += 1)
        if (getenv(names[k])) { fprintf(stderr, "render_image: DRT_LIGHT_LEVELS cannot be combined with %s\n", names[k]); return -1; }
    if (opt->features) { fprintf(stderr, "render_image: DRT_LIGHT_LEVELS cannot be combined with DRT_FEATURES\n"); return -1; }
    if (opt->mattes) { fprintf(stderr, "render_image: DRT_LIGHT_LEVELS cannot be combined with DRT_MATTES\n"); return -1; }
    for (const char *c = e;;)
    {
        char *end;
        const double level = strtod(c, &end);
        if (end == c || !isfinite(level) || (*end && *end != ','))
        { fprintf(stderr, "render_image: DRT_LIGHT_LEVELS=\"%s\": finite numbers separated by commas\n", e); return -1; }
        if (opt->n_levels == DRT_HOST_MAX_LEVELS) { fprintf(stderr, "render_image: DRT_LIGHT_LEVELS: %d levels at most\n", DRT_HOST_MAX_LEVELS); return -1; }
        opt->levels[opt->n_levels++] = level;
        if (!*end) break;
        c = end + 1;
    }
    return 0;
}

/* DRT_DEPTH_CUTS="d0,d1,..." (whole numbers from 1 to max_cast_depth, strictly ascending, DRT_MAX_DEPTH_CUTS at most): parsed and
 * checked here, before any device call, after the options it cannot be combined with. */
static int depth_cuts_options(const config_arguments *config, drt_host_options *opt)
{
    opt->n_depth_cuts = 0;
    const char *e = getenv("DRT_DEPTH_CUTS");
    if (!e) return 0;
    if (getenv("DRT_ADAPTIVE_ERROR")) { fprintf(stderr, "render_image: DRT_DEPTH_CUTS cannot be combined with DRT_ADAPTIVE_ERROR: an adaptive render keeps no cut films\n"); return -1; }
    if (getenv("DRT_CHECKPOINT_SPP")) { fprintf(stderr, "render_image: DRT_DEPTH_CUTS cannot be combined with DRT_CHECKPOINT_SPP: a checkpoint holds no cut films\n"); return -1; }
    if (getenv("DRT_RESUME")) { fprintf(stderr, "render_image: DRT_DEPTH_CUTS cannot be combined with DRT_RESUME: a checkpoint holds no cut films\n"); return -1; }
    if (getenv("DRT_TURNTABLE")) { fprintf(stderr, "render_image: DRT_DEPTH_CUTS cannot be combined with DRT_TURNTABLE\n"); return -1; }
    if (getenv("DRT_LIGHT_LEVELS")) { fprintf(stderr, "render_image: DRT_DEPTH_CUTS cannot be combined with DRT_LIGHT_LEVELS\n"); return -1; }
    for (const char *c = e;;)
    {
        if (*c < '0' || *c > '9')
        { fprintf(stderr, "render_image: DRT_DEPTH_CUTS=\"%s\": whole numbers separated by commas\n", e); return -1; }
        char *end;
        const unsigned long long d = strtoull(c, &end, 10);
        if (*end && *end != ',')
        { fprintf(stderr, "render_image: DRT_DEPTH_CUTS=\"%s\": whole numbers separated by commas\n", e); return -1; }
        if (opt->n_depth_cuts == DRT_MAX_DEPTH_CUTS) { fprintf(stderr, "render_image: DRT_DEPTH_CUTS: %d depths at most\n", DRT_MAX_DEPTH_CUTS); return -1; }
        if (d < 1 || d > config->max_cast_depth)
        { fprintf(stderr, "render_image: DRT_DEPTH_CUTS: depth %llu is not in 1..max_cast_depth (%u)\n", d, config->max_cast_depth); return -1; }
        if (opt->n_depth_cuts && (u32)d <= opt->depth_cuts[opt->n_depth_cuts - 1])
        { fprintf(stderr, "render_image: DRT_DEPTH_CUTS=\"%s\": the depths are not strictly ascending\n", e); return -1; }
        opt->depth_cuts[opt->n_depth_cuts++] = (u32)d;
        if (!*end) break;
        c = end + 1;
    }
    char path[64];
    const u32 deepest = opt->depth_cuts[opt->n_depth_cuts - 1];
    if (depth_path(path, config->output_spd, deepest, ".spd") || depth_path(path, config->average_spd, deepest, ".spd") ||
        depth_path(path, config->variance_spd, deepest, ".spd") || depth_path(path, config->output_spd, deepest, ".bmp"))
    { fprintf(stderr, "render_image: DRT_DEPTH_CUTS: an output name with .depth%u.spd behind it is longer than 63 characters\n", deepest); return -1; }
    return 0;
}

/* DRT_REGIONS="x,y,w,h:spp;x,y,w,h:spp;..." (whole numbers; DRT_HOST_MAX_REGIONS regions at most; a region has a size, begins inside
 * the image and asks for num_pixel_samples or more): parsed and checked here, before any device call. */
static int regions_options(const config_arguments *config, drt_host_options *opt)
{
    opt->n_regions = 0;
    const char *e = getenv("DRT_REGIONS");
    if (!e) return 0;
    static const char *const others[] = { "DRT_ADAPTIVE_ERROR", "DRT_CHECKPOINT_SPP", "DRT_RESUME", "DRT_TURNTABLE", "DRT_LIGHT_LEVELS", "DRT_DEPTH_CUTS", "DRT_PROJECTION" };
    for (size_t k = 0; k < sizeof(others) / sizeof(others[0]); k += 1)
        if (getenv(others[k])) { fprintf(stderr, "render_image: DRT_REGIONS cannot be combined with %s\n", others[k]); return -1; }
    static const char seps[4] = { ',', ',', ',', ':' };
    for (const char *c = e;;)
    {
        unsigned long long v[5];
        const char *end = c;
        int ok = 1;
        for (int k = 0; ok && k < 5; k += 1)
        {
            char *stop = NULL;
            ok = *end >= '0' && *end <= '9';
            if (!ok) break;
            v[k] = strtoull(end, &stop, 10);
            end = stop;
            ok = v[k] <= 0xFFFFFFFFull && (k == 4 || *end == seps[k]);
            if (ok && k < 4) end += 1;
        }
        if (!ok || (*end && *end != ';'))
        { fprintf(stderr, "render_image: DRT_REGIONS=\"%s\": regions x,y,w,h:spp of whole numbers, separated by semicolons\n", e); return -1; }
        if (opt->n_regions == DRT_HOST_MAX_REGIONS) { fprintf(stderr, "render_image: DRT_REGIONS: %d regions at most\n", DRT_HOST_MAX_REGIONS); return -1; }
        if (v[2] == 0 || v[3] == 0)
        { fprintf(stderr, "render_image: DRT_REGIONS: region %u (%llu,%llu,%llu,%llu) has no size\n", opt->n_regions, v[0], v[1], v[2], v[3]); return -1; }
        if (v[0] >= config->output_width || v[1] >= config->output_height)
        {
            fprintf(stderr, "render_image: DRT_REGIONS: region %u (%llu,%llu,%llu,%llu) lies outside the %u x %u image\n", opt->n_regions, v[0], v[1], v[2], v[3],
                    config->output_width, config->output_height);
            return -1;
        }
        if (v[4] == 0 || v[4] < config->num_pixel_samples)
        {
            fprintf(stderr, "render_image: DRT_REGIONS: region %u asks for %llu samples: num_pixel_samples (%u) or more\n", opt->n_regions, v[4],
                    config->num_pixel_samples);
            return -1;
        }
        for (int k = 0; k < 5; k += 1) opt->regions[opt->n_regions][k] = (u32)v[k];
        opt->n_regions += 1;
        if (!*end) break;
        c = end + 1;
    }
    if (strlen(config->output_spd) + strlen(".counts.bmp") > 63)
    { fprintf(stderr, "render_image: DRT_REGIONS: the output name with .counts.bmp behind it is longer than 63 characters\n"); return -1; }
    return 0;
}

/* DRT_SENSOR="a.csv,b.csv,..." (one curve per file, DRT_MAX_SENSOR_CHANNELS at most): parsed and checked here, before any device call,
 * after the options it cannot be combined with. The curves themselves are resampled once the scene has given the grid. */
static int sensor_options(const config_arguments *config, drt_host_options *opt)
{
    opt->n_sensor = 0;
    const char *e = getenv("DRT_SENSOR");
    if (!e) return 0;
    static const char *const others[] = { "DRT_ADAPTIVE_ERROR", "DRT_CHECKPOINT_SPP", "DRT_RESUME", "DRT_TURNTABLE", "DRT_LIGHT_LEVELS", "DRT_DEPTH_CUTS", "DRT_REGIONS" };
    for (size_t k = 0; k < sizeof(others) / sizeof(others[0]); k += 1)
        if (getenv(others[k])) { fprintf(stderr, "render_image: DRT_SENSOR cannot be combined with %s: that render keeps no sensor film\n", others[k]); return -1; }
    for (const char *c = e;;)
    {
        const char *end = strchr(c, ',');
        const size_t len = end ? (size_t)(end - c) : strlen(c);
        if (len == 0) { fprintf(stderr, "render_image: DRT_SENSOR=\"%s\": an empty entry (one CSV file per curve, separated by commas)\n", e); return -1; }
        if (opt->n_sensor == DRT_MAX_SENSOR_CHANNELS) { fprintf(stderr, "render_image: DRT_SENSOR: %d curves at most\n", DRT_MAX_SENSOR_CHANNELS); return -1; }
        if (len >= sizeof(opt->sensor_csv[0])) { fprintf(stderr, "render_image: DRT_SENSOR: a file name of %zu characters, %d at most\n", len, (int)sizeof(opt->sensor_csv[0]) - 1); return -1; }
        char *path = opt->sensor_csv[opt->n_sensor];
        memcpy(path, c, len);
        path[len] = 0;
        FILE *f = fopen(path, "rb");
        const int first = f ? fgetc(f) : EOF; /* (a directory opens, and cannot be read) */
        if (f) fclose(f);
        if (first == EOF) { fprintf(stderr, "render_image: DRT_SENSOR: cannot read %s\n", path); return -1; }
        opt->n_sensor += 1;
        if (!end) break;
        c = end + 1;
    }
    char path[64];
    if (sensor_path(path, config->output_spd, ".spd") || sensor_path(path, config->average_spd, ".spd") ||
        sensor_path(path, config->variance_spd, ".spd") || sensor_path(path, config->output_spd, ".bmp"))
    { fprintf(stderr, "render_image: DRT_SENSOR: an output name with .sensor.spd behind it is longer than 63 characters\n"); return -1; }
    return 0;
}

/* DRT_BUCKETS="n[,trim]" (whole numbers; 1 <= n <= DRT_MAX_BUCKETS; 2 * trim < n; no trim with n = 1, which has nothing to resolve):
 * parsed and checked here, before any device call. Without a trim the median's: (n - 1) / 2. */
static int buckets_options(const config_arguments *config, drt_host_options *opt)
{
    opt->n_buckets = opt->bucket_trim = 0;
    const char *e = getenv("DRT_BUCKETS");
    if (!e) return 0;
    static const char *const others[] = { "DRT_ADAPTIVE_ERROR", "DRT_CHECKPOINT_SPP", "DRT_RESUME", "DRT_TURNTABLE", "DRT_LIGHT_LEVELS", "DRT_DEPTH_CUTS", "DRT_SENSOR", "DRT_REGIONS" };
    for (size_t k = 0; k < sizeof(others) / sizeof(others[0]); k += 1)
        if (getenv(others[k])) { fprintf(stderr, "render_image: DRT_BUCKETS cannot be combined with %s: that render keeps no bucket films\n", others[k]); return -1; }
    unsigned long long v[2] = { 0, 0 };
    int n_values = 0, ok = 1;
    const char *c = e;
    for (; ok && n_values < 2; n_values += 1)
    {
        char *stop = NULL;
        ok = *c >= '0' && *c <= '9';
        if (!ok) break;
        v[n_values] = strtoull(c, &stop, 10);
        ok = v[n_values] <= 0xFFFFFFFFull && stop - c <= 10;
        c = stop;
        if (!ok || *c != ',') { n_values += 1; break; }
        c += 1;
        if (n_values == 1) ok = 0; /* a second comma */
    }
    if (!ok || *c || n_values == 0)
    { fprintf(stderr, "render_image: DRT_BUCKETS=\"%s\": n or n,trim in whole numbers\n", e); return -1; }
    if (v[0] == 0 || v[0] > DRT_MAX_BUCKETS) { fprintf(stderr, "render_image: DRT_BUCKETS: %llu buckets: from 1 to %d\n", v[0], DRT_MAX_BUCKETS); return -1; }
    if (n_values == 2 && v[0] == 1) { fprintf(stderr, "render_image: DRT_BUCKETS: one bucket has nothing to resolve, and so no trim\n"); return -1; }
    if (n_values == 2 && 2 * v[1] >= v[0])
    { fprintf(stderr, "render_image: DRT_BUCKETS: a trim of %llu leaves nothing of %llu buckets (2 * trim < n)\n", v[1], v[0]); return -1; }
    if (config->num_pixel_samples < v[0])
    { fprintf(stderr, "render_image: DRT_BUCKETS: %llu buckets of num_pixel_samples = %u samples: some bucket would stay empty\n", v[0], config->num_pixel_samples); return -1; }
    char path[64];
    if (bucket_path(path, config->output_spd, (u32)v[0] - 1, ".spd") || bucket_path(path, config->average_spd, (u32)v[0] - 1, ".spd") ||
        bucket_path(path, config->variance_spd, (u32)v[0] - 1, ".spd") || robust_path(path, config->average_spd, ".spd") ||
        robust_path(path, config->variance_spd, ".spd") || robust_path(path, config->output_spd, ".bmp"))
    { fprintf(stderr, "render_image: DRT_BUCKETS: an output name with .bucket%u.spd or .robust.spd behind it is longer than 63 characters\n", (u32)v[0] - 1); return -1; }
    opt->n_buckets = (u32)v[0];
    opt->bucket_trim = n_values == 2 ? (u32)v[1] : ((u32)v[0] - 1) / 2;
    return 0;
}

/* DRT_LOBES=standard|functions: a preset of lobe films, checked here, before any device call. The maps are those of pydrt.LOBE_PRESETS:
 * "functions" -- emission, then one film per scattering function in bdsf_list.h's order, direct and indirect together; "standard" --
 * emission; diffuse direct, indirect; glossy (bp_glossy, ct_conductor) direct, indirect; specular (mirror, fs_conductor, dielectric
 * reflectance); transmission. */
static int lobes_options(const config_arguments *config, drt_host_options *opt)
{
    static const char *const functions_names[] = { "emission", "bp_diffuse", "bp_glossy", "mirror", "fs_conductor", "fs_dielectric_reflectance",
                                                   "fs_dielectric_transmittance", "ct_conductor" };
    static const char *const standard_names[] = { "emission", "diffuse_direct", "diffuse_indirect", "glossy_direct", "glossy_indirect", "specular", "transmission" };
    opt->n_lobes = 0;
    opt->lobe_names = NULL;
    memset(&opt->lobe_map, 0, sizeof(opt->lobe_map));
    const char *e = getenv("DRT_LOBES");
    if (!e) return 0;
    static const char *const others[] = { "DRT_ADAPTIVE_ERROR", "DRT_CHECKPOINT_SPP", "DRT_RESUME", "DRT_TURNTABLE", "DRT_LIGHT_LEVELS", "DRT_DEPTH_CUTS", "DRT_SENSOR", "DRT_REGIONS", "DRT_BUCKETS" };
    for (size_t k = 0; k < sizeof(others) / sizeof(others[0]); k += 1)
        if (getenv(others[k])) { fprintf(stderr, "render_image: DRT_LOBES cannot be combined with %s: that render keeps no lobe films\n", others[k]); return -1; }
    drt_lobe_map m;
    memset(&m, 0, sizeof(m));
    u32 n = 0;
    if (strcmp(e, "functions") == 0)
    {
        n = 8;
        m.emission = 0;
        for (u32 f = 0; f < DRT_NUM_BDSFS; f += 1) m.direct[f] = m.indirect[f] = (uint8_t)(1 + f);
        opt->lobe_names = functions_names;
    }
    else if (strcmp(e, "standard") == 0)
    {
        n = 7;
        m.emission = 0;
        m.direct[DRT_BDSF_bp_diffuse_bdsf] = 1; m.indirect[DRT_BDSF_bp_diffuse_bdsf] = 2;
        m.direct[DRT_BDSF_bp_glossy_bdsf] = m.direct[DRT_BDSF_ct_conductor_bdsf] = 3;
        m.indirect[DRT_BDSF_bp_glossy_bdsf] = m.indirect[DRT_BDSF_ct_conductor_bdsf] = 4;
        m.direct[DRT_BDSF_mirror_bdsf] = m.indirect[DRT_BDSF_mirror_bdsf] = 5;
        m.direct[DRT_BDSF_fs_conductor_bdsf] = m.indirect[DRT_BDSF_fs_conductor_bdsf] = 5;
        m.direct[DRT_BDSF_fs_dielectric_reflectance_bdsf] = m.indirect[DRT_BDSF_fs_dielectric_reflectance_bdsf] = 5;
        m.direct[DRT_BDSF_fs_dielectric_transmittance_bdsf] = m.indirect[DRT_BDSF_fs_dielectric_transmittance_bdsf] = 6;
        opt->lobe_names = standard_names;
    }
    else { fprintf(stderr, "render_image: DRT_LOBES=\"%s\": standard or functions\n", e); return -1; }
    char path[64];
    if (lobe_path(path, config->output_spd, n - 1, ".spd") || lobe_path(path, config->average_spd, n - 1, ".spd") ||
        lobe_path(path, config->variance_spd, n - 1, ".spd") || lobe_path(path, config->output_spd, n - 1, ".bmp") || lobes_txt_path(path, config->output_spd))
    { fprintf(stderr, "render_image: DRT_LOBES: an output name with .lobe%u.spd or .lobes.txt behind it is longer than 63 characters\n", n - 1); return -1; }
    opt->n_lobes = n;
    opt->lobe_map = m;
    return 0;
}

void render_image(config_arguments *config)
{
    drt_host_options opt;
    memset(&opt, 0, sizeof(opt));
    const char *e;
    opt.seed = 1;
    if ((e = getenv("DRT_DEVICE"))) opt.device = atoi(e);
    if ((e = getenv("DRT_DEVICES")))
    {
        if (strcmp(e, "all") == 0) opt.all_devices = 1;
        else
            for (const char *c = e; *c && opt.n_devices < 16;)
            {
                char *end;
                long d = strtol(c, &end, 10);
                if (end == c) break;
                opt.devices[opt.n_devices++] = (int32_t)d;
                c = (*end == ',') ? end + 1 : end;
            }
    }
    if ((e = getenv("DRT_SEED"))) opt.seed = strtoull(e, NULL, 0);
    if ((e = getenv("DRT_BATCH_SPP"))) opt.batch_spp = (u32)atoi(e);
    if ((e = getenv("DRT_CHECKPOINT_SPP"))) opt.checkpoint_spp = (u32)atoi(e);
    if ((e = getenv("DRT_RESUME"))) opt.resume = (u32)atoi(e);
    if (adaptive_options(config, &opt) != 0) exit(-1);
    if (denoise_options(config, &opt) != 0) exit(-1);
    if (features_options(config, &opt) != 0) exit(-1);
    if (mattes_options(&opt) != 0) exit(-1);
    if (pick_options(config, &opt) != 0) exit(-1);
    if (projection_options(&opt) != 0) exit(-1);
    if (turntable_options(&opt) != 0) exit(-1);
    if (light_levels_options(&opt) != 0) exit(-1);
    if (depth_cuts_options(config, &opt) != 0) exit(-1);
    if (regions_options(config, &opt) != 0) exit(-1);
    if (sensor_options(config, &opt) != 0) exit(-1);
    if (buckets_options(config, &opt) != 0) exit(-1);
    if (lobes_options(config, &opt) != 0) exit(-1);
    if (render_image_ex(config, &opt, NULL) != 0) exit(-1);
}
