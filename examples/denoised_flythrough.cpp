// examples/denoised_flythrough.cpp -- the whole per-frame recipe of the real-time pipeline from C++:
// the camera is parked for the first frames and then walked by the scripted input of the interactive build
// (tyr_camera_handle_input: W held, the cursor two pixels right of the centre), and every frame goes through
//     tyr_set_camera; tyr_reset_accum; tyr_render_aov(1); tyr_render_motion against the previous camera; tyr_render(spp);
//     tyr_svgf(RESOLVE); tyr_taa
// with TYR_SVGF_RESET / TYR_TAA_RESET on the first frame.  Every K-th frame's anti-aliased picture goes to
// <prefix>_<frame>.ppm, and the mean milliseconds of each stage (hipEvent pairs on the ctx's stream) go to stdout.
//
// With --specular-guides[=K] (anywhere on the line; K = 8 bounces at most) the guides are taken behind mirrors and glass
// (INTEGRATION.md 4k): tyr_render_aov_chain instead of tyr_render_aov; tyr_svgf gets the chain's albedo, normal and depth and
// tyr_render_motion_chain's motion; tyr_taa, whose edges are the first surface's, gets depth_first and tyr_render_motion's.
//
//   denoised_flythrough [device] [frames = 32] [K = 8] [prefix = taa] [width = 640] [height = 360] [spp = 1] [parked = frames / 2]
//                       [--specular-guides[=K]]
#define TYRANT_IMPLEMENTATION
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "tyrant/interop.h"

using namespace tyrant;

#define TYR_CHECK(x)                                                                            \
	do {                                                                                        \
		int rc_ = (x);                                                                          \
		if (rc_) {                                                                              \
			std::fprintf(stderr, "tyr_assert: %s %s %d\n", tyr_status_string(rc_), __FILE__, __LINE__); \
			std::exit(rc_ > 0 && rc_ < 256 ? rc_ : 1);                                          \
		}                                                                                       \
	} while (0)

// a small height field standing in for Data/castle.ply (absent from the reference checkout), under the reference's spheres
static std::vector<vec3> make_mesh(int cells) {
	std::vector<vec3> v;
	auto P = [&](int i, int j) {
		const float x = -80.0f + 160.0f * i / cells, y = -80.0f + 160.0f * j / cells;
		return vec3{ x, y, -18.0f + 6.0f * std::sin(x * 0.09f) * std::cos(y * 0.08f) };
	};
	for (int j = 0; j < cells; ++j)
		for (int i = 0; i < cells; ++i) {
			const vec3 p00 = P(i, j), p10 = P(i + 1, j), p11 = P(i + 1, j + 1), p01 = P(i, j + 1);
			v.insert(v.end(), { p00, p10, p11, p00, p11, p01 });
		}
	return v;
}

template <class T>
static T* dev_array(size_t count) {
	void* p = nullptr;
	TYR_CHECK(hipMalloc(&p, count * sizeof(T)));
	return static_cast<T*>(p);
}

int main(int argc, char** argv) {
	int max_chain = -1; // -1: first-hit guides
	for (int i = 1; i < argc; ++i) {
		if (std::strncmp(argv[i], "--specular-guides", 17) != 0)
			continue;
		max_chain = argv[i][17] == '=' ? std::atoi(argv[i] + 18) : TYR_AOV_CHAIN_MAX;
		for (int j = i; j + 1 < argc; ++j)
			argv[j] = argv[j + 1];
		--argc;
		--i;
	}
	if (max_chain > TYR_AOV_CHAIN_MAX) {
		std::fprintf(stderr, "--specular-guides: at most %d bounces\n", TYR_AOV_CHAIN_MAX);
		return 2;
	}
	const bool chained = max_chain >= 0;
	const int device = argc > 1 ? std::atoi(argv[1]) : 0;
	const int frames = argc > 2 ? std::atoi(argv[2]) : 32;
	const int every = argc > 3 ? std::atoi(argv[3]) : 8;
	const std::string prefix = argc > 4 ? argv[4] : "taa";
	const unsigned W = argc > 5 ? static_cast<unsigned>(std::atoi(argv[5])) : 640u;
	const unsigned H = argc > 6 ? static_cast<unsigned>(std::atoi(argv[6])) : 360u;
	const unsigned spp = argc > 7 ? static_cast<unsigned>(std::atoi(argv[7])) : 1u;
	const int parked = argc > 8 ? std::atoi(argv[8]) : frames / 2;
	if (frames < 1 || W < 1 || H < 1 || spp < 1) {
		std::fprintf(stderr, "usage: denoised_flythrough [device] [frames] [K] [prefix] [width] [height] [spp] [parked] [--specular-guides[=K]]\n");
		return 2;
	}
	const size_t n = static_cast<size_t>(W) * H;

	tyr_config cfg{};
	cfg.width = W;
	cfg.height = H;
	cfg.queue_size = 262144;
	cfg.device = device;
	cfg.nranks = 1;
	tyr_ctx* ctx = nullptr;
	TYR_CHECK(tyr_create(&ctx, &cfg));
	TYR_CHECK(tyr_set_blit_buffer(ctx, nullptr)); // the ctx allocates and owns the accumulation buffer
	Scene scene;
	scene.Load(ctx, make_mesh(96));
	TYR_CHECK(hipSetDevice(device));

	float* albedo = dev_array<float>(3 * n);
	float* normal = dev_array<float>(3 * n);
	float* depth = dev_array<float>(n);
	int32_t* prim = dev_array<int32_t>(n);
	int32_t* geom = dev_array<int32_t>(n);
	float* motion = dev_array<float>(2 * n);
	float* prev_depth = dev_array<float>(n);
	float* filtered = dev_array<float>(4 * n); // tyr_svgf's resolved frame
	float* screen = dev_array<float>(4 * n);   // tyr_taa's
	// --specular-guides: sample 0's chain, and what tyr_taa keeps of the first surface
	int32_t* chain = chained ? dev_array<int32_t>(n) : nullptr;
	float* length0 = chained ? dev_array<float>(n) : nullptr;
	float* depth_first = chained ? dev_array<float>(n) : nullptr;
	float* motion_first = chained ? dev_array<float>(2 * n) : nullptr;
	float* prev_depth_first = chained ? dev_array<float>(n) : nullptr;
	std::vector<float> host(4 * n);

	enum { AOV, MOTION, RENDER, SVGF, TAA, STAGES };
	const char* const stage_name[STAGES] = { "render_aov", "render_motion", "render", "svgf", "taa" };
	hipEvent_t ev[STAGES + 1];
	for (hipEvent_t& e : ev)
		TYR_CHECK(hipEventCreate(&e));
	double ms_sum[STAGES] = {};

	tyr_camera_pose pose{ { 0.0f, -250.0f, 95.0f }, { 1.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.0f }, 0.0, -0.273 };
	auto camera_of = [](const tyr_camera_pose& p) {
		tyr_camera c{};
		TYR_CHECK(tyr_camera_update(p.horizontal_angle, p.vertical_angle, c.direction));
		for (int k = 0; k < 3; ++k) {
			c.position[k] = p.position[k];
			c.up[k] = p.up[k];
		}
		c.focalDistance = 1.0f;
		c.lensRadius = 0.0f;
		return c;
	};
	// the interactive build's input path: W held, the cursor 2 px right of the centre, 1 / 60 s per frame
	tyr_input_state input{};
	input.key_w = 1;
	input.window_w = static_cast<int32_t>(W);
	input.window_h = static_cast<int32_t>(H);
	input.cursor_x = W * 0.5 + 2.0;
	input.cursor_y = H * 0.5;

	tyr_camera prev_cam = camera_of(pose);
	unsigned pictures = 0;
	for (int f = 0; f < frames; ++f) {
		if (f >= parked)
			TYR_CHECK(tyr_camera_handle_input(&pose, &input, 1.0 / 60.0));
		const tyr_camera cam = camera_of(pose);
		if (f == 0)
			prev_cam = cam;
		TYR_CHECK(tyr_set_camera(ctx, &cam));
		TYR_CHECK(tyr_reset_accum(ctx));

		TYR_CHECK(hipEventRecord(ev[AOV], nullptr));
		const tyr_aov_out aov{ albedo, normal, depth, prim, geom };
		if (chained) {
			const tyr_aov_chain_out ext{ chain, nullptr, nullptr, length0, depth_first };
			TYR_CHECK(tyr_render_aov_chain(ctx, 1, static_cast<uint32_t>(max_chain), &aov, &ext, nullptr));
		} else {
			TYR_CHECK(tyr_render_aov(ctx, 1, &aov, nullptr));
		}
		TYR_CHECK(tyr_sync(ctx)); // the events below are recorded on the null stream: keep it in step with the ctx's
		TYR_CHECK(hipEventRecord(ev[MOTION], nullptr));
		const tyr_motion_in min{ prim, geom, &prev_cam, nullptr };
		const tyr_motion_out mout{ motion, prev_depth };
		if (chained) { // the virtual image's motion for the filter, the first surface's for the anti-aliasing
			const tyr_motion_chain_in via{ chain, length0 };
			const tyr_motion_out first{ motion_first, prev_depth_first };
			TYR_CHECK(tyr_render_motion_chain(ctx, &min, &via, &mout, nullptr));
			TYR_CHECK(tyr_render_motion(ctx, &min, &first, nullptr));
		} else {
			TYR_CHECK(tyr_render_motion(ctx, &min, &mout, nullptr));
		}
		TYR_CHECK(tyr_sync(ctx));
		TYR_CHECK(hipEventRecord(ev[RENDER], nullptr));
		TYR_CHECK(tyr_render(ctx, spp, UINT32_MAX, nullptr));
		TYR_CHECK(hipEventRecord(ev[SVGF], nullptr));
		const tyr_svgf_in sin{ nullptr, albedo, normal, depth, motion, prev_depth };
		// the defaults (DESIGN.md "SVGF"), plus the tone map
		const tyr_svgf_params sp{ 8, 0.05f, 0.9f, 3, 2.0f, 0.02f, 7, TYR_SVGF_RESOLVE | (f == 0 ? TYR_SVGF_RESET : 0u) };
		TYR_CHECK(tyr_svgf(ctx, &sin, &sp, filtered, nullptr, nullptr));
		TYR_CHECK(tyr_sync(ctx));
		TYR_CHECK(hipEventRecord(ev[TAA], nullptr));
		const tyr_taa_in tin{ filtered, chained ? depth_first : depth, chained ? motion_first : motion, chained ? prev_depth_first : prev_depth };
		const tyr_taa_params tp{ 0.2f, 1.5f, f == 0 ? TYR_TAA_RESET : 0u }; // the defaults (DESIGN.md "Temporal anti-aliasing")
		TYR_CHECK(tyr_taa(ctx, &tin, &tp, screen, nullptr));
		TYR_CHECK(tyr_sync(ctx));
		TYR_CHECK(hipEventRecord(ev[STAGES], nullptr));
		TYR_CHECK(hipEventSynchronize(ev[STAGES]));
		for (int s = 0; s < STAGES; ++s) {
			float ms = 0.f;
			TYR_CHECK(hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
			ms_sum[s] += ms;
		}
		if (every > 0 && (f + 1) % every == 0) {
			TYR_CHECK(hipMemcpy(host.data(), screen, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
			const std::string name = prefix + "_" + std::to_string(f + 1) + ".ppm";
			TYR_CHECK(tyr_write_ppm(name.c_str(), host.data(), W, H));
			++pictures;
		}
		prev_cam = cam;
	}
	std::printf("%d frames of %u x %u at %u spp, the camera parked for the first %d:", frames, W, H, spp, parked < frames ? parked : frames);
	double total = 0.0;
	for (int s = 0; s < STAGES; ++s) {
		std::printf(" %s %.3f ms", stage_name[s], ms_sum[s] / frames);
		total += ms_sum[s] / frames;
	}
	std::printf("; %.3f ms per frame (each stage timed to its end: a viewer would not wait between them)\n", total);
	tyr_counters k;
	TYR_CHECK(tyr_get_counters(ctx, &k));
	std::printf("%u pictures as %s_<frame>.ppm; device_error %u\n", pictures, prefix.c_str(), k.device_error);
	if (chained)
		std::printf("specular guides: max_chain %d\n", max_chain);
	const int rc = k.device_error ? 1 : 0;
	for (hipEvent_t& e : ev)
		(void)hipEventDestroy(e);
	TYR_CHECK(tyr_destroy(ctx));
	for (void* p : { static_cast<void*>(albedo), static_cast<void*>(normal), static_cast<void*>(depth), static_cast<void*>(prim), static_cast<void*>(geom), static_cast<void*>(motion),
	                 static_cast<void*>(prev_depth), static_cast<void*>(filtered), static_cast<void*>(screen), static_cast<void*>(chain), static_cast<void*>(length0),
	                 static_cast<void*>(depth_first), static_cast<void*>(motion_first), static_cast<void*>(prev_depth_first) })
		(void)hipFree(p);
	return rc;
}
