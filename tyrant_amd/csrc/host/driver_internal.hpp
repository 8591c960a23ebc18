// driver_internal.hpp -- what the translation units behind the C ABI share (private to the library).  host/driver.cpp owns the ctx
// (create / destroy, scene, setters, the accumulation buffer) and defines these helpers; host/render_loop.cpp is launch_kernels' loop
// (tyr_launch_kernels, tyr_render one iteration ahead of the counts); host/staged_api.cpp the test hooks (tyr_stage_*, AoS queue
// import / export); host/tuning_probes.cpp tyr_set_tuning, the timings and the device / layout probes.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ctx.hpp"
#include "host.hpp"

#define HIPCHK(expr)                       \
	do {                                   \
		hipError_t e_ = (expr);            \
		if (e_ != hipSuccess)              \
			return static_cast<int>(e_);   \
	} while (0)

namespace tyr {
namespace drv {

template <class T>
int dev_alloc(T*& p, size_t count) {
	void* v = nullptr;
	hipError_t e = hipMalloc(&v, count * sizeof(T));
	if (e != hipSuccess)
		return e == hipErrorOutOfMemory ? TYR_ERR_OOM : static_cast<int>(e);
	p = static_cast<T*>(v);
	return TYR_OK;
}
template <class T>
void dev_free(T*& p) {
	if (p)
		(void)hipFree(p);
	p = nullptr;
}

int alloc_rayq(RayQ& q, size_t n);
void free_rayq(RayQ& q);
void default_spheres(tyr_sphere* s);
bool finite_n(const float* p, int n);
int use_device(tyr_ctx* c);
int sync_counters(tyr_ctx* c);
int push_counters(tyr_ctx* c);
// the scene as a launch sees it (the render's and the queries' alike): the top of the tree staged as far as the tuning allows
DevScene launch_scene(const tyr_ctx* c);
FrameParams make_params(const tyr_ctx* c);
void collect_timings_of(tyr_ctx* c, int set);
void collect_timings(tyr_ctx* c);
uint32_t planned_new(const tyr_ctx* c);
int stage_begin(tyr_ctx* c);
// split (enqueue_primary and enqueue_trace of one iteration alike): null, or the camera window by which the top-up is made in two
// parts -- enqueue_primary then launches the window's part on the ctx's stream and the rest on its second one, and enqueue_trace leaves
// that one room beside its traversal kernel and has the ctx's stream wait for it behind that kernel
void enqueue_primary(tyr_ctx* c, const FrameParams& P, uint32_t nNew, const PrimaryWindow* split = nullptr);
void enqueue_extend(tyr_ctx* c, const FrameParams& P0, uint32_t nLive, uint32_t nSurvivors);
void enqueue_trace(tyr_ctx* c, const FrameParams& P0, uint32_t nLive, uint32_t nSurvivors, uint32_t maxShadowPrev, const PrimaryWindow* split = nullptr);
// host/primary_window.cpp: the ctx's camera window, brought up to date; and the window to make a merged iteration's top-up of at
// most nNew rays in two parts by (behind at most nSurvivors survivors), or null when it is to be one k_primary
void primary_window_update(tyr_ctx* c);
// ... the same from its inputs alone (tyr_primary_window_probe): the rectangle in the frame's pixels and in the rank's rows; false = the whole frame
bool primary_window_of(const tyr_camera& cam, uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks, const float rootMin[3], const float rootMax[3], int inset, uint32_t rect[4], PrimaryWindow& local);
const PrimaryWindow* primary_split(tyr_ctx* c, uint32_t nNew, uint32_t nSurvivors);
void enqueue_shade(tyr_ctx* c, const FrameParams& P, uint32_t nLive);
void enqueue_connect(tyr_ctx* c, const FrameParams& P0, uint32_t maxShadow);
bool merged_render(const tyr_ctx* c);
int flush_pending_shadow(tyr_ctx* c);
void stage_end(tyr_ctx* c);
int check_device_error(const tyr_ctx* c);
// enter(): makes the ctx's device current; the caller's is restored on the way out (tyr_query_*, tyr_scene_refit and the frame
// filters, as tyr_bvh_build_device does)
struct DeviceScope {
	int prev = -1;
	int enter(tyr_ctx* c) {
		HIPCHK(hipGetDevice(&prev));
		return use_device(c);
	}
	~DeviceScope() {
		if (prev >= 0)
			(void)hipSetDevice(prev);
	}
};
// host/refit.cpp: keep what tyr_scene_refit needs of the scene just uploaded (TYR_FLAG_REFIT).  nodes: the reference's array on
// the host, or null (then read back from dNodes); dNodes: the same on the device, or null (then copied from nodes); slotNode /
// pairNode: the layout pass's maps on the host, or dSlotNode on the device (adopted: freed or kept, null on return)
int refit_keep(tyr_ctx* c, const tyr_bvh_node* nodes, const tyr_bvh_node* dNodes, int32_t nNodes, const int32_t* slotNode, int32_t*& dSlotNode, uint32_t nSlots,
               const int32_t* pairNode, uint32_t nPairSides);
void refit_free(tyr_ctx* c);
// host/winding.cpp: (re)build the moment tree of the scene the ctx holds (TYR_FLAG_WINDING; nothing without it) from the reference's
// node array -- dNodes on the device, or null (then staged from hostNodes) -- and the ctx's triangle records, on the ctx's
// stream, which is idle on return
int winding_build(tyr_ctx* c, const tyr_bvh_node* dNodes, const tyr_bvh_node* hostNodes, int32_t nNodes);
void winding_free(tyr_ctx* c);
// host/signed.cpp: wait for the last tyr_bake_sdf; free its near-brick list and event (tyr_destroy)
void sdf_free(tyr_ctx* c);
// host/query.cpp: wait for the ctx's queries in flight on any stream; free their device words (tyr_destroy)
int query_wait(tyr_ctx* c);
// ... and the bracket round every launch of a query-like pass (tyr_query_*, tyr_render_aov, tyr_render_motion) on the caller's
// `stream` (NULL: the ctx's).  open() goes in front of the launch: it makes the ctx's device current (the caller's comes back
// when the object goes, on every way out), takes the stream's entry and clears its chunk ticket word on s.  close() goes behind
// it: the launch's error, then the stream's `done` event, which tyr_query_error, tyr_scene_refit and tyr_destroy wait for.  An
// entry with several launches opens and closes once per launch; work enqueued behind a close() needs a close() of its own.
struct QueryLaunch {
	hipStream_t s = nullptr;
	uint32_t* ticket = nullptr;
	int open(tyr_ctx* c, void* stream);
	int close();

private:
	DeviceScope scope;
	hipEvent_t done = nullptr;
};
// the fields every query's Params share, for a launch that is open
template <class P>
auto query_spheres(P& p, const tyr_ctx* c, int) -> decltype((void)p.spheres) {
	std::memcpy(p.spheres, c->spheres, sizeof(p.spheres));
}
template <class P>
void query_spheres(P&, const tyr_ctx*, long) {}
template <class P>
void query_fields(P& p, const tyr_ctx* c, const QueryLaunch& L) {
	p.scene = launch_scene(c);
	query_spheres(p, c, 0);
	p.ticket = L.ticket;
	p.error = c->dQuery;
}
// host/driver.cpp: the camera basis of the staged prologue (kernel.cu:699-700) for the ctx's current camera
void camera_basis(const tyr_ctx* c, float right[3], float up[3]);
// ... and for any camera at the ctx's width and height (tyr_render_motion's previous camera)
void camera_basis(const tyr_ctx* c, const tyr_camera& cam, float right[3], float up[3]);
void camera_basis(uint32_t width, uint32_t height, const tyr_camera& cam, float right[3], float up[3]);
void query_free(tyr_ctx* c);
// host/denoise.cpp: the bracket round the launch of a frame pass (tyr_denoise, tyr_temporal, tyr_svgf, tyr_taa,
// tyr_allocate_samples) on the caller's `stream` (NULL: the ctx's), once its arguments have been accepted.  The pass's buffers
// belong to the ctx, so its calls are ordered by the event in its FilterState.  open() goes in front of the launch: it makes
// the ctx's device current (the caller's comes back when the object goes, on every way out), creates the event on first use
// and has s wait for the previous call (a no-op before the first record).  close() goes behind it: the launch's error, then
// the event; a pass that asked for its history() now has history `next` as the last call's output.  An error on the way
// leaves the state as it was.
struct FilterLaunch {
	hipStream_t s = nullptr;
	uint32_t prev = 0, next = 0; // history(): the history the last call wrote and the one this call writes
	int open(tyr_ctx* c, FilterState& state, void* stream);
	// a buffer of the pass, allocated on first use; with a fresh one there is no history
	template <class T>
	int buffer(T*& p, size_t count) {
		if (p)
			return TYR_OK;
		st->have = false;
		return dev_alloc(p, count);
	}
	// sets prev and next; true: history prev is to be read (the pass has one and the call does not reset it)
	bool history(bool reset) {
		pingPong = true;
		prev = st->cur;
		next = prev ^ 1u;
		return st->have && !reset;
	}
	int close();

private:
	DeviceScope scope;
	FilterState* st = nullptr;
	bool pingPong = false;
};
// ... wait for the last call of every pass; free their events and buffers (tyr_destroy)
void filters_free(tyr_ctx* c);
// the limits and checks that the passes' parameters share
constexpr uint32_t kMaxHistory = 1024, kMaxPasses = 8, kMaxNormalPowerLog2 = 10;
bool positive_finite(float v);
// max_history, depth_tolerance and normal_cos of tyr_temporal and tyr_svgf
bool reprojection_ok(uint32_t maxHistory, float depthTolerance, float normalCos);
// host/adaptive.cpp: free the sample map's ticket list and scratch (tyr_destroy)
void adaptive_free(tyr_ctx* c);
// AoS import / export (host/staged_api.cpp): physical slots that hold a record, per segment counter array `seg` (device pointer)
int valid_slots(const uint32_t* dSeg, std::vector<uint32_t>& slots, uint32_t* total = nullptr);
void dense_counts(uint32_t n, uint32_t* cnt /* [kSegs * kSegStride] */);
template <class T>
int gather(const T* dev, const std::vector<uint32_t>& slots, uint32_t extent, std::vector<T>& out) {
	std::vector<T> all(extent);
	if (extent)
		HIPCHK(hipMemcpy(all.data(), dev, extent * sizeof(T), hipMemcpyDeviceToHost));
	out.resize(slots.size());
	for (size_t i = 0; i < slots.size(); ++i)
		out[i] = all[slots[i]];
	return TYR_OK;
}

} // namespace drv
} // namespace tyr
