// mjb_ray.h — the engine's one definition of the ray - primitive intersection: the step kernel's rangefinder sensor (mjb_step.hip, MJB_SENS_RANGEFINDER)
// and the batched ray kernel (mjb_ray.hip) both include it, so that a ray cast either way reads the same bits.
#pragma once

#include "../../include/mjb.h"
#include "mjb_math.h"

// mju_rayGeom for the engine's primitives (engine_ray.c; oracle/mjo_smooth.c ray_geom): distance along pnt + x vec, -1 for no hit
DEVI double ray_quad(double a, double b, double c, double &x0, double &x1)
{
	double det = b * b - a * c;
	if (det < MJB_MINVAL) { x0 = x1 = -1; return -1; }
	det = sqrt(det);
	x0 = (-b - det) / a;
	x1 = (-b + det) / a;
	return x0 >= 0 ? x0 : (x1 >= 0 ? x1 : -1.0);
}
DEVI double ray_geom(const double *pos, const double *mat, const double *size, const double *pnt, const double *vec, int type)
{
	const double dif[3] = { pnt[0] - pos[0], pnt[1] - pos[1], pnt[2] - pos[2] };
	double lp[3], lv[3], x0, x1;
	matTvec3(lp, mat, dif);
	matTvec3(lv, mat, vec);
	if (type == MJB_GEOM_PLANE) {
		if (lv[2] > -MJB_MINVAL) return -1;
		const double x = -lp[2] / lv[2];
		if (x < 0) return -1;
		const double p0 = lp[0] + x * lv[0], p1 = lp[1] + x * lv[1];
		return ((size[0] <= 0 || fabs(p0) <= size[0]) && (size[1] <= 0 || fabs(p1) <= size[1])) ? x : -1.0;
	}
	if (type == MJB_GEOM_SPHERE) return ray_quad(dot3(lv, lv), dot3(lv, lp), dot3(lp, lp) - size[0] * size[0], x0, x1);
	if (type == MJB_GEOM_CAPSULE) {
		double x = -1;
		const double sol = ray_quad(lv[0] * lv[0] + lv[1] * lv[1], lv[0] * lp[0] + lv[1] * lp[1], lp[0] * lp[0] + lp[1] * lp[1] - size[0] * size[0], x0, x1);
		if (sol >= 0 && fabs(lp[2] + sol * lv[2]) <= size[1]) x = sol;
		for (int side = 1; side >= -1; side -= 2) {
			const double ld[3] = { lp[0], lp[1], lp[2] - side * size[1] };
			ray_quad(dot3(lv, lv), dot3(lv, ld), dot3(ld, ld) - size[0] * size[0], x0, x1);
			if (x0 >= 0 && side * (lp[2] + x0 * lv[2]) >= size[1] && (x < 0 || x0 < x)) x = x0;
			if (x1 >= 0 && side * (lp[2] + x1 * lv[2]) >= size[1] && (x < 0 || x1 < x)) x = x1;
		}
		return x;
	}
	if (type == MJB_GEOM_BOX) {
		double x = -1;
		for (int i = 0; i < 3; i++) {
			if (fabs(lv[i]) <= MJB_MINVAL) continue;
			const int j = (i + 1) % 3, k = (i + 2) % 3;
			for (int side = -1; side <= 1; side += 2) {
				const double sol = (side * size[i] - lp[i]) / lv[i];
				if (sol >= 0 && fabs(lp[j] + sol * lv[j]) <= size[j] && fabs(lp[k] + sol * lv[k]) <= size[k] && (x < 0 || sol < x)) x = sol;
			}
		}
		return x;
	}
	return -1;
}
