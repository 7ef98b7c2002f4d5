/*
 * drt_window_rule.h -- the live window: the rectangle of image pixels outside which no camera ray can reach the scene.
 *
 * Plain C++, no HIP: the launcher and the host-only entry point drt_live_window_of share it. DESIGN.md section 3 has the proof.
 *
 * The pinhole camera (camera_ray, drt_kernels.h) starts a ray at the film point
 *     P = film_bottom_left + (x + px) pixel_width right + (y + py) pixel_height up,   px, py in [0, 1],
 * and sends it through the aperture position A. Every point a surface's intersector can report lies in the scene's padded box B
 * (prim_bounds). If B is wholly in front of A and the film wholly behind it, a ray meets B only beyond A, and the film points whose
 * rays do are the projection of B through A onto the film plane: a convex set, inside the bounding rectangle of its eight projected
 * corners. The window is that rectangle in pixel units, rounded outwards, plus one whole guard pixel on every side.
 */
#ifndef DRT_WINDOW_RULE_H
#define DRT_WINDOW_RULE_H

#include <cmath>
#include <cstdint>

#include "drt_hip.h"

struct LiveWindow
{
    uint32_t x_lo, x_hi, y_lo, y_hi; /* image pixels [x_lo, x_hi) x [y_lo, y_hi); x_lo == x_hi: empty */
    bool     whole;                  /* the rule does not apply: the window is the whole tile */
};

static inline double lw_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static inline double lw_det(const double a[3], const double b[3], const double c[3]) /* columns a, b, c */
{
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - b[0] * (a[1] * c[2] - a[2] * c[1]) + c[0] * (a[1] * b[2] - a[2] * b[1]);
}

static inline LiveWindow live_window_whole(const drt_params &p)
{
    const uint32_t stride = p.row_stride ? p.row_stride : 1u;
    LiveWindow w = {p.x0, p.x0 + p.tile_w, p.y0, p.tile_h ? p.y0 + (p.tile_h - 1u) * stride + 1u : p.y0, true};
    return w;
}

/* lo, hi: the box of everything the scene's intersectors can accept (already padded as prim_bounds pads it); escape_dark: a ray that
 * leaves the scene is worth +0 at every wavelength (the escape material is a black body that does not emit). */
static inline LiveWindow live_window_rule(const double lo[3], const double hi[3], const drt_camera &cam, const drt_params &p, bool escape_dark)
{
    const LiveWindow whole = live_window_whole(p);
    if (!escape_dark || !(cam.aperture_radius <= 0.0)) return whole; /* (a NaN radius: whole) */
    if (!(cam.pixel_width > 0.0) || !(cam.pixel_height > 0.0) || !std::isfinite(cam.pixel_width) || !std::isfinite(cam.pixel_height)) return whole;
    double extent = 0.0;
    for (int k = 0; k < 3; k += 1)
    {
        const double v[6] = {lo[k], hi[k], cam.aperture_position[k], cam.film_bottom_left[k], cam.forward[k], cam.right[k]};
        for (int i = 0; i < 6; i += 1)
        {
            if (!std::isfinite(v[i])) return whole;
            extent = std::fmax(extent, std::fabs(v[i]));
        }
        if (!std::isfinite(cam.up[k]) || !(lo[k] <= hi[k])) return whole;
    }
    if (!(extent < 0x1p100)) return whole;
    const double pad = 4.0 * 0x1p-20 * extent; /* on top of prim_bounds' own: the device's ray is the rounded one */
    /* the film wholly behind the pinhole: its four corners */
    const double fw = (double)p.width * cam.pixel_width, fh = (double)p.height * cam.pixel_height;
    for (int c = 0; c < 4; c += 1)
    {
        double q[3];
        for (int k = 0; k < 3; k += 1)
            q[k] = cam.film_bottom_left[k] + ((c & 1) ? fw : 0.0) * cam.right[k] + ((c & 2) ? fh : 0.0) * cam.up[k] - cam.aperture_position[k];
        if (!(lw_dot(q, cam.forward) < 0.0)) return whole;
    }
    /* corner C of the padded box: a right + b up + t (C - A) = A - film_bottom_left, t > 0; the film point is (a, b) */
    double rhs[3];
    for (int k = 0; k < 3; k += 1) rhs[k] = cam.aperture_position[k] - cam.film_bottom_left[k];
    double xmin = HUGE_VAL, xmax = -HUGE_VAL, ymin = HUGE_VAL, ymax = -HUGE_VAL;
    for (int c = 0; c < 8; c += 1)
    {
        double d[3];
        for (int k = 0; k < 3; k += 1) d[k] = (((c >> k) & 1) ? hi[k] + pad : lo[k] - pad) - cam.aperture_position[k];
        if (!(lw_dot(d, cam.forward) >= pad) || !(lw_dot(d, cam.forward) > 0.0)) return whole; /* not in front of the pinhole by the pad */
        const double det = lw_det(cam.right, cam.up, d);
        const double a = lw_det(rhs, cam.up, d) / det, b = lw_det(cam.right, rhs, d) / det, t = lw_det(cam.right, cam.up, rhs) / det;
        if (!std::isfinite(a) || !std::isfinite(b) || !(t > 0.0) || !std::isfinite(t)) return whole;
        const double x = a / cam.pixel_width, y = b / cam.pixel_height;
        if (!std::isfinite(x) || !std::isfinite(y)) return whole;
        xmin = std::fmin(xmin, x); xmax = std::fmax(xmax, x);
        ymin = std::fmin(ymin, y); ymax = std::fmax(ymax, y);
    }
    /* pixel x covers film abscissae [x, x + 1] (both draws' ends included): it is live when that meets [xmin, xmax], which is
     * ceil(xmin) - 1 <= x <= floor(xmax). One guard pixel more on every side; then the tile's own bounds */
    const double gx0 = std::ceil(xmin) - 2.0, gx1 = std::floor(xmax) + 2.0, gy0 = std::ceil(ymin) - 2.0, gy1 = std::floor(ymax) + 2.0;
    auto clip = [](double v, uint32_t a, uint32_t b) -> uint32_t { return v <= (double)a ? a : v >= (double)b ? b : (uint32_t)v; };
    LiveWindow w = {clip(gx0, whole.x_lo, whole.x_hi), clip(gx1, whole.x_lo, whole.x_hi), clip(gy0, whole.y_lo, whole.y_hi),
                    clip(gy1, whole.y_lo, whole.y_hi), false};
    if (w.x_lo >= w.x_hi || w.y_lo >= w.y_hi) w.x_lo = w.x_hi = w.y_lo = w.y_hi = 0; /* the scene is wholly off the tile */
    return w;
}

#endif
