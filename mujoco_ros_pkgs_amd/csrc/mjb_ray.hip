// mjb_ray.hip -- batched ray casting (mjb_rays_*): mj_ray for many rays of every env in one launch, fp64.
//
// One lane casts one (env, ray) pair against the env's geoms with ray_geom of mjb_ray.h, the function the step kernel's rangefinder
// sensor calls: the smallest x >= 0 wins, strict `<` in geom order, so the lower geom id keeps a tie.  A block of up to 256 lanes covers
// `epb` whole envs (a ray set shorter than a block: a lidar ring) or a tile of 256 rays of one env (an image).  The geom loop is the same
// for every lane of a block, so the block stages the geoms through LDS in tiles of MJB_RAY_TILE / epb geoms per env -- pose and size as one
// 128-byte record, type and body beside it -- and the lanes of an env then read identical addresses, which the LDS serves as a broadcast; the ray
// loop itself issues no global load.  The tile is a fixed number of records: no model is refused for its ngeom, and since every lane
// still walks its env's geoms in ascending order, no result depends on the tile or on the shape of the launch.
// Nothing is culled ahead of ray_geom: a geom is skipped only by the rules of the interface (mask / alpha 0, the ray's own body).
#include <hip/hip_runtime.h>

#include "mjb_dev.h"
#include "mjb_math.h"
#include "mjb_ray.h"

namespace {

constexpr int RAY_BLOCK = 256;
constexpr int REC = 16;  // doubles per staged geom: xpos[3] xmat[9] size[3] and one of padding (16-byte aligned records); type and body sit in an int2 beside them
static_assert(MJB_RAY_TILE <= 64 && MJB_RAY_TILE * (REC * sizeof(double) + sizeof(int2)) == 8704, "geom tile of the ray kernel: 64 records of 128 + 8 bytes");

// tab: pnt[3][nray] | vec[3][nray] (doubles), then {site, exclude}[nray] and visible[ngeom] (ints)
__global__ void __launch_bounds__(RAY_BLOCK) mjb_ray_kernel(const KernelParams MJB_AS4 *__restrict__ P, const double *__restrict__ tab, int nray, int epb, int rays_per_block,
                                                            int ray_blocks, double *__restrict__ dist_out, int *__restrict__ geomid_out)
{
	__shared__ double tile[MJB_RAY_TILE * REC];
	__shared__ int2 tile_tb[MJB_RAY_TILE];  // type (-1: not a geom this launch looks at), body
	const DevModel MJB_AS4 &m = P->m;
	const DevState MJB_AS4 &s = P->s;
	const FrameLayout MJB_AS4 &L = P->L;
	const int nenv = s.nenv, ngeom = m.ngeom;
	const int *__restrict__ itab = reinterpret_cast<const int *>(tab + (size_t)6 * nray);
	const int *__restrict__ visible = itab + (size_t)2 * nray;
	const int env_block = (int)(blockIdx.x / (unsigned int)ray_blocks), ray_block = (int)(blockIdx.x % (unsigned int)ray_blocks);
	const int env0 = env_block * epb;
	const int t = (int)threadIdx.x;
	const int le = t / rays_per_block;  // this lane's env within the block, and its ray
	const int ray = ray_block * rays_per_block + (t - le * rays_per_block);
	const int env = env0 + le;
	const bool live = le < epb && env < nenv && ray < nray;
	const int tg = MJB_RAY_TILE / epb;  // geoms per env and tile

	double org[3] = { 0, 0, 0 }, dir[3] = { 0, 0, 1 };
	int skip = -1;
	if (live) {
		const double pnt[3] = { tab[ray], tab[(size_t)nray + ray], tab[(size_t)2 * nray + ray] };
		const double vec[3] = { tab[(size_t)3 * nray + ray], tab[(size_t)4 * nray + ray], tab[(size_t)5 * nray + ray] };
		const int site = itab[2 * ray], excl = itab[2 * ray + 1];
		if (site >= 0) {
			const double *f = s.frame_ws + (size_t)env * s.frame_stride;
			double SM[9], sp[3], rp[3];
			ld9(SM, f + L.site_xmat + 9 * site);
			ld3(sp, f + L.site_xpos + 3 * site);
			matvec3(rp, SM, pnt);
			matvec3(dir, SM, vec);
			for (int k = 0; k < 3; k++) org[k] = sp[k] + rp[k];
			if (excl) skip = m.site_bodyid[site];
		} else {
			for (int k = 0; k < 3; k++) { org[k] = pnt[k]; dir[k] = vec[k]; }
		}
	}

	double dist = -1;
	int hit = -1;
	for (int g0 = 0; g0 < ngeom; g0 += tg) {
		__syncthreads();  // (the previous tile has been read)
		for (int idx = t; idx < epb * tg * REC; idx += (int)blockDim.x) {
			const int rec = idx / REC, fld = idx - rec * REC;
			const int re = rec / tg, g = g0 + (rec - re * tg), e = env0 + re;
			const bool ok = e < nenv && g < ngeom;
			double v = 0;
			if (fld == REC - 1) {
				int2 tb = { -1, -1 };
				if (ok && visible[g]) {
					tb.x = s.env_geom_type ? s.env_geom_type[(size_t)e * ngeom + g] : m.geom_type[g];
					tb.y = m.geom_bodyid[g];
				}
				tile_tb[rec] = tb;
			} else if (ok) {
				const double *f = s.frame_ws + (size_t)e * s.frame_stride;
				if (fld < 3) v = f[L.geom_xpos + 3 * g + fld];
				else if (fld < 12) v = f[L.geom_xmat + 9 * g + (fld - 3)];
				else v = s.env_geom_size ? s.env_geom_size[((size_t)e * ngeom + g) * 3 + (fld - 12)] : m.geom_size[3 * g + (fld - 12)];
			}
			tile[idx] = v;
		}
		__syncthreads();
		if (live) {
			const int n = min(tg, ngeom - g0);
			const double *rec = tile + (size_t)le * tg * REC;
			const int2 *tb = tile_tb + le * tg;
			for (int j = 0; j < n; j++, rec += REC) {
				const int gt = tb[j].x, gb = tb[j].y;
				if (gt < 0 || gb == skip) continue;
				double gp[3], gm[9], gs[3];
				ld3(gp, rec);
				ld9(gm, rec + 3);
				ld3(gs, rec + 12);
				const double x = ray_geom(gp, gm, gs, org, dir, gt);
				if (x >= 0 && (x < dist || dist < 0)) {
					dist = x;
					hit = g0 + j;
				}
			}
		}
	}
	if (live) {
		dist_out[(size_t)env * nray + ray] = dist;
		geomid_out[(size_t)env * nray + ray] = hit;
	}
}

// the shape of a launch: whole envs per block while a ray set is no longer than half a block, else tiles of one env's rays
void ray_launch_shape(int nray, int *epb, int *rays_per_block)
{
	int e = RAY_BLOCK / nray;
	if (e > MJB_RAY_TILE) e = MJB_RAY_TILE;
	if (e < 1) e = 1;
	*epb = e;
	*rays_per_block = e > 1 ? nray : (nray < RAY_BLOCK ? nray : RAY_BLOCK);
}

}  // namespace

int mjb_launch_rays(const KernelParams *Pdev, const double *tab, int nenv, int nray, double *dist, int *geomid, void *stream)
{
	int epb, rpb;
	ray_launch_shape(nray, &epb, &rpb);
	const long long ray_blocks = (nray + rpb - 1) / rpb, env_blocks = (nenv + epb - 1) / epb;
	if (ray_blocks * env_blocks > 0x7fffffffLL) return (int)hipErrorInvalidConfiguration;
	const int threads = (epb * rpb + 63) & ~63;  // (whole wavefronts; at most RAY_BLOCK)
	hipLaunchKernelGGL(mjb_ray_kernel, dim3((unsigned int)(ray_blocks * env_blocks)), dim3((unsigned int)threads), 0, (hipStream_t)stream, (const KernelParams MJB_AS4 *)Pdev, tab, nray, epb,
	                   rpb, (int)ray_blocks, dist, geomid);
	return (int)hipGetLastError();
}
