/*
 * ppf_camera_math.h — the camera model of ppf_camera (include/ppf_hip.h): rational radial + tangential distortion in
 * OpenCV's coefficient order, forward (project) and inverse (unproject, Newton's method with the analytic Jacobian).
 *
 * Like ppf_detmath.h this is the single numeric specification both sides evaluate: the host entries ppf_camera_project /
 * ppf_camera_unproject / ppf_camera_map_boxes and the kernels k_reg_rays / k_reg_draw call the functions below, and
 * tests/register_oracle.py restates them in numpy operation for operation.  Only IEEE-754 fp64 + - * / and comparisons,
 * evaluated as written, left to right; nothing may be fused, so every translation unit including this file is compiled
 * with -ffp-contract=off.
 */
#ifndef PPF_CAMERA_MATH_H
#define PPF_CAMERA_MATH_H

#include "ppf_detmath.h" /* PPF_HD, ppf_d2bits, ppf_bits2d, the contraction pragmas */
#include "ppf_hip.h"     /* ppf_camera, PPF_CAMERA_NEWTON_ITERS */

#define PPF_CAMERA_MAX_RESIDUAL 1e-18 /* (dxd)^2 + (dyd)^2 of an accepted unprojection, normalised units squared */

PPF_HD int ppf_cam_finite(double x) { return (ppf_d2bits(x) & 0x7ff0000000000000ULL) != 0x7ff0000000000000ULL; }
PPF_HD double ppf_cam_nan(void) { return ppf_bits2d(0x7ff8000000000000ULL); } /* numpy's nan */

/* x*x + y*y > max_r*max_r, with max_r 0 for no limit */
PPF_HD int ppf_cam_over_max_r(const ppf_camera* c, double x, double y) {
  return c->max_r != 0.0 && x * x + y * y > c->max_r * c->max_r;
}

/* normalised (x, y) -> distorted normalised (xd, yd); J (may be NULL) receives the partials
 * {dxd/dx, dxd/dy, dyd/dx, dyd/dy}.  Returns b != 0. */
PPF_HD int ppf_cam_distort(const ppf_camera* c, double x, double y, double* xd, double* yd, double* J) {
  const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
  const double a = 1.0 + c->k1 * r2 + c->k2 * r4 + c->k3 * r6;
  const double b = 1.0 + c->k4 * r2 + c->k5 * r4 + c->k6 * r6;
  const double d = a / b;
  *xd = x * d + 2.0 * c->p1 * x * y + c->p2 * (r2 + 2.0 * x * x);
  *yd = y * d + c->p1 * (r2 + 2.0 * y * y) + 2.0 * c->p2 * x * y;
  if (J) {
    const double a1 = c->k1 + 2.0 * c->k2 * r2 + 3.0 * c->k3 * r4; /* da / dr2 */
    const double b1 = c->k4 + 2.0 * c->k5 * r2 + 3.0 * c->k6 * r4; /* db / dr2 */
    const double d1 = (a1 * b - a * b1) / (b * b);                 /* dd / dr2 */
    const double dx = d1 * (2.0 * x), dy = d1 * (2.0 * y);         /* dd / dx, dd / dy */
    J[0] = d + x * dx + 2.0 * c->p1 * y + 6.0 * c->p2 * x;
    J[1] = x * dy + 2.0 * c->p1 * x + 2.0 * c->p2 * y;
    J[2] = y * dx + 2.0 * c->p1 * x + 2.0 * c->p2 * y;
    J[3] = d + y * dy + 6.0 * c->p1 * y + 2.0 * c->p2 * x;
  }
  return b != 0.0 && ppf_cam_finite(d);
}

/* normalised (x, y) -> pixel (u, v).  Returns 0 and (NaN, NaN) for an invalid point: b == 0, a / b, u or v not finite,
 * or the point over max_r. */
PPF_HD int ppf_cam_project(const ppf_camera* c, double x, double y, double* u, double* v) {
  double xd, yd;
  int ok = ppf_cam_distort(c, x, y, &xd, &yd, (double*)0);
  const double uu = c->fx * xd + c->cx, vv = c->fy * yd + c->cy;
  ok = ok && ppf_cam_finite(uu) && ppf_cam_finite(vv) && !ppf_cam_over_max_r(c, x, y);
  *u = ok ? uu : ppf_cam_nan();
  *v = ok ? vv : ppf_cam_nan();
  return ok;
}

/* pixel (u, v) -> normalised (x, y): PPF_CAMERA_NEWTON_ITERS Newton steps from (xd, yd), no early exit.  Returns 0 and
 * (NaN, NaN) for an invalid ray: a determinant of 0, b == 0 or a / b not finite at the result, x, y or the final residual
 * not finite, a residual above PPF_CAMERA_MAX_RESIDUAL (a folded-over solution), or the result over max_r. */
PPF_HD int ppf_cam_unproject(const ppf_camera* c, double u, double v, double* xo, double* yo) {
  const double xd = (u - c->cx) / c->fx, yd = (v - c->cy) / c->fy;
  double x = xd, y = yd, fx, fy, J[4];
  int ok = 1;
  for (int it = 0; it < PPF_CAMERA_NEWTON_ITERS; it++) {
    (void)ppf_cam_distort(c, x, y, &fx, &fy, J);
    const double e0 = fx - xd, e1 = fy - yd;
    const double det = J[0] * J[3] - J[1] * J[2];
    if (det == 0.0) ok = 0;
    x = x - (J[3] * e0 - J[1] * e1) / det;
    y = y - (J[0] * e1 - J[2] * e0) / det;
  }
  const int bok = ppf_cam_distort(c, x, y, &fx, &fy, (double*)0);
  const double e0 = fx - xd, e1 = fy - yd;
  const double res = e0 * e0 + e1 * e1;
  ok = ok && bok && ppf_cam_finite(x) && ppf_cam_finite(y) && ppf_cam_finite(res) && res <= PPF_CAMERA_MAX_RESIDUAL &&
       !ppf_cam_over_max_r(c, x, y);
  *xo = ok ? x : ppf_cam_nan();
  *yo = ok ? y : ppf_cam_nan();
  return ok;
}

#endif /* PPF_CAMERA_MATH_H */
