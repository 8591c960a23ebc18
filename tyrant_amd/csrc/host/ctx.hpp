// ctx.hpp -- tyr_ctx, the state behind the C ABI's opaque handle (private to the library: host/driver.cpp owns it,
// host/dist.cpp reads the stream, the blit buffer and the sharding from it).
#pragma once

#include <vector>

#include <hip/hip_runtime.h>

#include "../hip/refit.hpp"
#include "../hip/winding.hpp"
#include "host.hpp"

using tyr::ConnectCounters;
using tyr::DevCounters;
using tyr::DevScene;
using tyr::LaunchCache;
using tyr::RayQ;
using tyr::ShadowQ;
using tyr::SunParams;
using tyr::Tuning;

// What a frame pass (tyr_denoise, tyr_temporal, tyr_svgf, tyr_taa, tyr_allocate_samples) keeps between calls beside its buffers,
// which belong to the ctx (host/driver_internal.hpp FilterLaunch).  done: the event behind the last call (the next one waits for
// it, on whatever stream).  The passes with a history keep two and alternate: history cur is the last call's output, valid only
// when have is set.
struct FilterState {
	hipEvent_t done = nullptr;
	uint32_t cur = 0;
	bool have = false;
};

struct tyr_ctx {
	tyr_config cfg{};
	hipStream_t stream = nullptr;
	bool ownStream = false;
	uint32_t localRows = 0, localPixels = 0;

	RayQ q[2]{};
	int cur = 0; // q[cur] = work queue, q[cur ^ 1] = next (the caller's std::swap, main.cpp:169)
	ShadowQ shadow[2]{}; // iteration i writes and connects shadow[i & 1]
	DevCounters* dK = nullptr;
	DevCounters* hK = nullptr; // pinned host mirror
	DevCounters* hSnap[2] = { nullptr, nullptr }; // tyr_render one iteration ahead: where the counters of iteration i land (set i & 1)
	hipEvent_t evSnap[2] = { nullptr, nullptr };
	tyr::HostSnap* hostSnap[2] = { nullptr, nullptr }; // TYR_TUNE_KERNEL_SNAPSHOT: written by k_shade's last block (pinned, device-visible)
	tyr::HostSnap* hostSnapDev[2] = { nullptr, nullptr }; // ... as the device addresses them
	uint32_t snapSeq = 0;                               // stamp of the last iteration queued with a kernel-written snapshot
	uint32_t snapSeqOf[2] = { 0, 0 };                   // ... per set (0: that iteration uses the copy + event)
	ConnectCounters* dKc = nullptr; // two sets, iteration i uses set i & 1
	uint32_t iter = 0;
	uint32_t shadowSet = 0; // which of the two sets holds the counts of the shadow queue's current content (tyr_shadow_export)

	hipEvent_t evSnapshot = nullptr;
	// A top-up in two parts (host/primary_window.cpp): the lowest-priority stream k_primary_rest runs on beside the
	// traversal launch, the event it waits for (k_primary_window has left it the plan) and the event behind it (the ctx's stream waits
	// for it right behind the traversal launch: whatever follows there follows the whole top-up)
	hipStream_t sideStream = nullptr;
	hipEvent_t evWindowDone = nullptr, evRestDone = nullptr;
	// the camera window and what it was computed from (recomputed when that changes, not per render)
	struct WindowKey {
		tyr_camera cam;
		float rootMin[3], rootMax[3];
		uint32_t rootRef;
		int inset;
	} windowKey{};
	bool windowValid = false;
	bool windowWhole = true;       // the window is the whole frame (or empty): a top-up is one k_primary
	uint32_t windowRect[4] = { 0, 0, 0, 0 }; // x0, x1, y0, y1 in the frame's pixels
	tyr::PrimaryWindow window{};   // ... and in the rank's own rows
	uint32_t primarySplits = 0;    // top-ups launched in two parts since tyr_create (tyr_primary_window_info.splits)
	// TYR_TUNE_SCAN_IN_TRACE
	bool scanCarried = false;      // the last shade launch left its slot scan to the next traversal launch (hip/scan_wave.hpp)
	uint32_t scanCarriedSet = 0;
	// tyr_render with TYR_TUNE_MERGE_TRACE: the shadow rays of the last shaded iteration have not been traced yet (they
	// ride in the next iteration's trace launch, or in a connect of their own when the render ends)
	bool shadowPending = false;
	uint32_t shadowPendingMax = 0;
	// tyr_render one iteration ahead: the last queued iteration turned out to be empty; once the stream is idle the device's
	// counters get back what that iteration's set_wavefront_globals zeroed (the live and shadow counts of the last real one)
	bool runAheadUndo = false;
	uint32_t undoLive = 0, undoShadows = 0;
	// hip/kernels.hpp "Queues": room per queue segment, the survive bytes and the two sets of scan tables
	uint32_t segCap = 0;
	uint8_t* survFlag = nullptr;
	unsigned long long* vWord[2] = { nullptr, nullptr };
	uint32_t* vPre[2] = { nullptr, nullptr };
	uint32_t* vBlk[2] = { nullptr, nullptr };
	bool unboundedRender = false; // tyr_render was called without an iteration limit: contributions may arrive an iteration early (TYR_TUNE_RETIRE_SKY's survivors)
	bool lastShadeFolded = false; // the shade launch that filled the current work / shadow queues did the sphere pre-passes' work too (TYR_TUNE_FOLD_SPHERES)
	float4* blit = nullptr;
	bool ownBlit = false;

	float4* dNodes = nullptr;
	float4* dQuads = nullptr;
	float4* dTris = nullptr;
	uint32_t* dLights = nullptr; // TYR_FLAG_LIGHT_LIST: emissive triangles, array order
	uint32_t nLights = 0;
	float triEmission[3] = { 3.0f, 3.0f, 3.0f }; // kernel.cu:680
	float4* dPalette = nullptr;                   // TYR_FLAG_TRIANGLE_COLORS: 256 x { colour, emission }
	DevScene scene{};
	bool haveScene = false;
	double uploadLayoutS = 0.0, uploadCopyS = 0.0; // the last tyr_scene_upload: host layout passes, allocation + copies to HBM (tyr_scene_info)
	bool layoutOnDevice = false; // ... and where its layout pass ran

	tyr_sphere spheres[TYR_NUM_SPHERES]{};
	tyr_camera cam{};
	float sunPos[2] = { 0.05f, 0.3f }; // variables.cpp:3
	bool sunChanged = true;             // variables.cpp:4
	SunParams sun{};

	// launch_kernels statics, kernel.cu:665-667, 688-691
	bool firstTime = true;
	uint32_t frame = 1;
	float lastPos[3] = { 0, 0, 0 }, lastDir[3] = { 0, 0, 0 };
	float lastFocal = 1.0f, lastLens = 0.02f;
	float camRight[3]{}, camUp[3]{};

	Tuning tuning{};
	LaunchCache launchCache{}; // occupancy answers of the persistent kernels, per ctx (not process-wide)
	int numCUs = 256;

	// tyr_query_* (host/query.cpp): their own device words -- the error bits, then a ring of chunk tickets, one per launch --
	// and one event per stream they ran on (what tyr_query_error, a scene change and tyr_destroy wait for).  No render state.
	struct QueryStream {
		hipStream_t stream;
		hipEvent_t done;   // recorded behind this stream's last query
		uint32_t word;     // its ticket word
		uint64_t lastUse;
	};
	uint32_t* dQuery = nullptr;
	uint64_t querySeq = 0;
	std::vector<QueryStream> queryStreams;

	// tyr_denoise (host/denoise.cpp): scratch for width * height pixels -- two illumination buffers, then the packed guide --
	// allocated by the first call
	float4* dDenoise = nullptr;
	FilterState denoise;

	// tyr_temporal (host/temporal.cpp): two histories of width * height pixels, each a (u.xyz, length) plane then a (normal.xyz,
	// depth) plane, allocated by the first call
	float4* dTemporal = nullptr;
	FilterState temporal;

	// tyr_svgf (host/svgf.cpp): two histories of width * height pixels, each a (u.xyz, length) plane then a (normal.xyz, depth)
	// plane (dSvgfHist), and a (m1, m2) plane (dSvgfMom).  dSvgfIllum: the a-trous passes' two (u.xyz, variance) buffers.  All
	// allocated by the first call
	float4* dSvgfHist = nullptr;
	float2* dSvgfMom = nullptr;
	float4* dSvgfIllum = nullptr;
	FilterState svgf;

	// tyr_taa (host/taa.cpp): two planes of width * height (rgb, validity) pixels, allocated by the first call
	float4* dTaaHist = nullptr;
	FilterState taa;

	// tyr_set_sample_map / tyr_allocate_samples (host/adaptive.cpp): the sample map's ticket list (4 bytes per ticket, grown as needed),
	// its length T and whether the camera rays take their pixels from it (mapped mode: until tyr_set_budget / tyr_render set a
	// budget of their own); the list build's scratch -- the map at the local pixels, the summary + histogram the host reads back,
	// the compaction's block counts -- and the allocator's (two 64-bit scans and three words), with its state
	uint32_t* dTickets = nullptr;
	uint64_t ticketCap = 0;
	uint32_t ticketTotal = 0;
	bool mapped = false;
	uint32_t* dMapScratch = nullptr;
	unsigned long long* dAllocScratch = nullptr;
	FilterState alloc;

	// TYR_FLAG_REFIT: what every scene upload keeps for tyr_scene_refit (host/refit.cpp)
	tyr::RefitPlan refit{};
	// TYR_FLAG_WINDING: the moment tree every scene upload and refit builds for tyr_query_winding (host/winding.cpp)
	tyr::WindingTree winding{};
	// tyr_bake_sdf (host/signed.cpp): the near-brick list -- word 0 the count, then sdfListCap brick indices -- kept from call to
	// call and grown as needed, and the event behind the last bake, which the next one waits for (they share the list)
	uint32_t* dSdfList = nullptr;
	size_t sdfListCap = 0;
	hipEvent_t sdfDone = nullptr;

	hipEvent_t ev[2][2 * TYR_K_COUNT]{}; // TYR_FLAG_PROFILE: start / stop per stage, two sets (iteration i uses set i & 1: two iterations may be queued)
	bool evUsed[2][TYR_K_COUNT]{};
	bool evEmpty[2][TYR_K_COUNT]{}; // TYR_TUNE_STAGE_TIMING: the stage launched nothing, its events are bound to no launch
	tyr_timings timings{};
};

