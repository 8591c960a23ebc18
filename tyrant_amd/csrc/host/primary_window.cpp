// primary_window.cpp -- the camera window: the pixel rectangle outside which no camera ray can pass the root box of the scene's
// tree, and the decision to make a top-up in two parts by it: the window's rays in front of the iteration's
// traversal launch, all the others beside it.  The window is a bound for scheduling, not for results: k_primary_rest traces a
// ray that passes the root box after all (hip/frame.hip trace_stray).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "driver_internal.hpp"

namespace tyr {
namespace drv {

namespace {

// [x0, x1) x [y0, y1) in the frame's pixels; false: the whole frame (one of the cases below, or nothing to gain)
bool project_root_box(const tyr_camera& cam, uint32_t width, uint32_t height, const float rootMin[3], const float rootMax[3], int inset, uint32_t rect[4]) {
	const double W = width, H = height;
	if (cam.lensRadius != 0.0f) // a thin lens: the rays of a pixel start all over the lens (no bound derived for it)
		return false;
	bool inside = true;
	for (int k = 0; k < 3; ++k)
		inside = inside && cam.position[k] >= rootMin[k] && cam.position[k] <= rootMax[k];
	if (inside)
		return false;
	// camera_focus (hip/device_common.hpp): direction ~ fwd + ndcX * right + ndcY * up with ndcX = jx / W - 0.5,
	// ndcY = (H - jy) / H - 0.5 and (jx, jy) the pixel minus its jitter; right and up are orthogonal to fwd and to each other
	// (camera_basis), so a point p in front of the camera plane is seen at ndc = (v.right / |right|^2, v.up / |up|^2) / (v.fwd / |fwd|^2),
	// v = p - position.  All eight corners in front: the box's picture is the convex hull of theirs.
	float rf[3], uf[3];
	camera_basis(width, height, cam, rf, uf);
	const double f[3] = { cam.direction[0], cam.direction[1], cam.direction[2] }, r[3] = { rf[0], rf[1], rf[2] }, u[3] = { uf[0], uf[1], uf[2] };
	auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
	const double ff = dot(f, f), rr = dot(r, r), uu = dot(u, u);
	double jx0 = HUGE_VAL, jx1 = -HUGE_VAL, jy0 = HUGE_VAL, jy1 = -HUGE_VAL;
	for (int corner = 0; corner < 8; ++corner) {
		double v[3];
		for (int k = 0; k < 3; ++k)
			v[k] = static_cast<double>((corner >> k) & 1 ? rootMax[k] : rootMin[k]) - cam.position[k];
		const double a = dot(v, f) / ff;
		if (!(a > 0.0)) // on or behind the camera plane (or not a number: a degenerate basis)
			return false;
		const double jx = (dot(v, r) / rr / a + 0.5) * W, jy = H - (dot(v, u) / uu / a + 0.5) * H;
		if (!std::isfinite(jx) || !std::isfinite(jy))
			return false;
		jx0 = std::min(jx0, jx), jx1 = std::max(jx1, jx), jy0 = std::min(jy0, jy), jy1 = std::max(jy1, jy);
	}
	// a pixel lies within one pixel of its jittered position (stratified_sample); one more pixel for the rounding of the device's
	// binary32 arithmetic and of the slab test
	const double grow = 2.0 - inset;
	const double x0 = std::min(std::max(std::floor(jx0) - grow, 0.0), W), x1 = std::min(std::max(std::floor(jx1) + 1.0 + grow, 0.0), W);
	const double y0 = std::min(std::max(std::floor(jy0) - grow, 0.0), H), y1 = std::min(std::max(std::floor(jy1) + 1.0 + grow, 0.0), H);
	if (!(x0 < x1 && y0 < y1)) // the box is out of the picture (or the inset ate the window)
		return false;
	rect[0] = static_cast<uint32_t>(x0), rect[1] = static_cast<uint32_t>(x1), rect[2] = static_cast<uint32_t>(y0), rect[3] = static_cast<uint32_t>(y1);
	return !(rect[0] == 0 && rect[1] == width && rect[2] == 0 && rect[3] == height);
}

} // namespace

bool primary_window_of(const tyr_camera& cam, uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks, const float rootMin[3], const float rootMax[3], int inset, uint32_t rect[4], PrimaryWindow& local) {
	if (!project_root_box(cam, width, height, rootMin, rootMax, inset, rect))
		return false;
	// rows y = yl * nranks + rank of this rank (hip/frame.hip primary_rays)
	const uint32_t localRows = height / nranks;
	auto row = [&](uint32_t y) { return y <= rank ? 0u : std::min((y - rank + nranks - 1) / nranks, localRows); };
	local = PrimaryWindow{ rect[0], rect[1], row(rect[2]), row(rect[3]) };
	return local.yl0 < local.yl1; // (false: none of the window's rows is this rank's)
}

void primary_window_update(tyr_ctx* c) {
	tyr_ctx::WindowKey key{};
	key.cam = c->cam;
	std::memcpy(key.rootMin, c->scene.rootMin, 12);
	std::memcpy(key.rootMax, c->scene.rootMax, 12);
	key.rootRef = c->scene.rootRef;
	key.inset = c->tuning.windowInset;
	if (c->windowValid && std::memcmp(&key, &c->windowKey, sizeof key) == 0)
		return;
	c->windowKey = key;
	c->windowValid = true;
	c->windowWhole = c->scene.rootRef == kRefDone || !primary_window_of(c->cam, c->cfg.width, c->cfg.height, c->cfg.rank, c->cfg.nranks, c->scene.rootMin, c->scene.rootMax, key.inset, c->windowRect, c->window);
	if (c->windowWhole) {
		c->windowRect[0] = c->windowRect[2] = 0, c->windowRect[1] = c->cfg.width, c->windowRect[3] = c->cfg.height;
		c->window = PrimaryWindow{ 0, c->cfg.width, 0, c->localRows };
	}
}

const PrimaryWindow* primary_split(tyr_ctx* c, uint32_t nNew, uint32_t nSurvivors) {
	if (c->tuning.primaryOverlap == 0 || c->mapped || c->scanCarried || nNew == 0)
		return nullptr;
	// Worth it where the traversal launch is thin -- it carries the window's rays and little else, a render's first launch -- and the
	// top-up large: beside a launch fat with survivors the other part only takes issue slots from it (profiles/primary_overlap_ab.txt)
	const uint64_t minNew = static_cast<uint64_t>(c->tuning.overlapMinNew);
	if (minNew != 0 && (nNew < minNew || static_cast<uint64_t>(nSurvivors) * 4 > nNew))
		return nullptr;
	primary_window_update(c);
	if (c->windowWhole)
		return nullptr;
	const PrimaryWindow& w = c->window;
	const uint64_t per = static_cast<uint64_t>(w.x1 - w.x0) * (w.yl1 - w.yl0);
	if (per * 2 > c->localPixels) // most of the frame is window: the traversal launch would wait for most of the top-up anyway
		return nullptr;
	// Room in the queue segments (tyr_create's segCap): a segment takes an eighth of each PART's blocks now, 256 rays more than an
	// eighth of its rays from each, on top of the survivors it holds (at most N / 8 + 1024 of them, and never more than there are)
	const uint64_t N = c->cfg.queue_size, sweeps = (static_cast<uint64_t>(c->localPixels) + nNew - 2) / c->localPixels + 1;
	const uint64_t inWindow = std::min<uint64_t>(per * sweeps, nNew);
	if (std::min<uint64_t>(nSurvivors, N / 8 + 1024) + nNew / 8 + inWindow / 8 + 2 * 256 + 2 > c->segCap)
		return nullptr;
	return &c->window;
}

} // namespace drv
} // namespace tyr

extern "C" int tyr_primary_window_probe(const tyr_camera* cam, uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks, const float root_min[3], const float root_max[3], int inset, tyr_primary_window_info* out) {
	if (!cam || !root_min || !root_max || !out || width == 0 || height == 0 || nranks == 0 || rank >= nranks || (height % nranks) != 0)
		return TYR_ERR_INVALID;
	uint32_t rect[4];
	tyr::PrimaryWindow local{};
	const bool part = tyr::drv::primary_window_of(*cam, width, height, rank, nranks, root_min, root_max, inset, rect, local);
	*out = tyr_primary_window_info{};
	out->whole_frame = part ? 0u : 1u;
	out->x0 = part ? rect[0] : 0u, out->x1 = part ? rect[1] : width, out->y0 = part ? rect[2] : 0u, out->y1 = part ? rect[3] : height;
	out->local_y0 = part ? local.yl0 : 0u, out->local_y1 = part ? local.yl1 : height / nranks;
	return TYR_OK;
}
