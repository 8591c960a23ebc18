// frame.hip -- the per-frame kernels around the traversal: primary_rays (kernel.cu:247-297),
// set_wavefront_globals (kernel.cu:227-244), the sphere halves of intersect_scene / intersect_scene_simple
// (kernel.cu:125-136, 168-172) as coherent pre-passes, blit_onto_framebuffer (kernel.cu:648-662).
#include "device_common.hpp"
#include "prologue.hpp"

namespace tyr {

// ======================================================================================
// primary_rays, kernel.cu:247-297.  One thread per new queue slot.
// ======================================================================================
// Four kernels share the body.  k_primary makes a whole top-up.  k_primary_window and k_primary_rest make it in two parts
// (DESIGN.md 4.8 (6)): the rays whose pixel lies in the camera window -- the only ones that can pass the root box, so the
// only ones the iteration's traversal launch reads -- and, beside that launch on a second stream, all the others.  A ray is
// the same ray whichever of the three makes it: its ticket `index` gives it its seed, its pixel and its virtual slot.
// k_primary_mapped makes a whole top-up of adaptive sampling (include/tyr_c.h "Adaptive sampling"): the pixel comes from the
// sample map's ticket list instead of the raster cursor, everything else is k_primary's.
enum : int { kPrimaryWhole = 0, kPrimaryWindow = 1, kPrimaryRest = 2, kPrimaryMapped = 3 };

// A ray of k_primary_rest that does pass the root box (the window is a bound the host computed, not something the result may
// rest on): the traversal launch is already running and does not know of it, so it is traced here -- the quad tree in the
// reference's visit order with the closest-hit accept rule, as hip/query_common.hpp q_traverse does it -- and queued with its
// answer.  One ray at a time per wave, on the wave's own 64-entry LDS stack (bvh.h:124): this is a path for a handful of rays.
// Why a walk of its own and neither of the two there are: bvh_closest (hip/traverse.hpp) walks the PAIR nodes, which a ctx of
// the merged path does not have on the device (tyr_scene_upload lays them out only for the counting and BVH_DEBUG flags: 64 MB on
// C3); q_traverse is a wave-wide state machine over LdsStack<12>, 24 KB of LDS per block plus 52 private entries per lane --
// scratch, and LDS that k_primary_rest's blocks need to fit beside the traversal launch's.  What has to stay in step with those
// two is the push order (farthest hit first), the pop test and the leaf's accept rule; tests/test_primary_overlap.py holds them to
// the oracle with the window shrunk, tests/fuzz_primary_overlap.py on random scenes.
struct WaveStack {
	uint2* entry;
	int n;
	bool overflow;
	__device__ __forceinline__ void push(bool on, uint32_t r, float t) {
		if (!on)
			return;
		if (n < kStackSize)
			entry[n++] = make_uint2(r, __float_as_uint(t));
		else
			overflow = true;
	}
};
__device__ __forceinline__ float2 trace_stray(const DevScene& sc, uint2* stack, f3 origin, f3 direction, float2 hitRecord, bool& overflow) {
	const RayConst r = make_ray(origin, direction);
	WaveStack st{ stack, 0, false };
	float dist = hitRecord.x;
	uint32_t ref = sc.quadRootRef;
	while (ref != kRefDone) {
		if (ref == kRefPop) {
			ref = kRefDone;
			while (st.n > 0) {
				const uint2 e = st.entry[--st.n];
				if (__uint_as_float(e.y) < dist) { // the pop-time half of Bbox.h:61
					ref = e.x;
					break;
				}
			}
		} else if ((int)ref >= 0) {
			const QuadHits h = test_quad<false, true>(sc.quads, ref, r, dist);
			const bool h0 = lane_in(h.hit[0]), h1 = lane_in(h.hit[1]), h2 = lane_in(h.hit[2]), h3 = lane_in(h.hit[3]);
			st.push(h3 && (h0 || h1 || h2), h.ref[3], h.t[3]);
			st.push(h2 && (h0 || h1), h.ref[2], h.t[2]);
			st.push(h1 && h0, h.ref[1], h.t[1]);
			ref = h0 ? h.ref[0] : h1 ? h.ref[1] : h2 ? h.ref[2] : h3 ? h.ref[3] : kRefPop;
		} else { // a leaf: bvh.h:129-140
			const uint32_t off = ref & (kMaxPrimOffset - 1);
			const uint32_t cnt = ((ref >> 26) & 31u) + 1u;
			for (uint32_t i = 0; i < cnt; ++i) {
				const float t = triangle_test(triangle_load(sc.tris, off + i), r);
				if (t > kEpsilon && t < dist && ((dist - t) > kEpsilon)) {
					hitRecord = make_float2(t, __uint_as_float(off + i));
					dist = t;
				}
			}
			ref = kRefPop;
		}
	}
	overflow = overflow || st.overflow;
	return hitRecord;
}

template <int PART>
__device__ __forceinline__ void primary_rays(const FrameParams& P, const PrimaryWindow& win, const MappedPrimary& map = MappedPrimary{}) {
	__shared__ uint32_t baseSh[kClasses], cntSh[8], lastSh;
	__shared__ uint2 strayStack[PART == kPrimaryRest ? (kBlock / 64) * kStackSize : 1];
	uint32_t index = blockIdx.x * kBlock + threadIdx.x;
	uint32_t cnt, nNew, start;
	unsigned long long budget = 0ull;
	if (PART == kPrimaryRest) {
		cnt = P.k->plan_cnt, nNew = P.k->plan_new, start = P.k->plan_start;
	} else {
		cnt = P.k->primary_ray_cnt; // survivors already in the buffer (kernel.cu:253)
		const unsigned long long room = (unsigned long long)(P.N - cnt);
		budget = P.k->budget_remaining;
		nNew = (uint32_t)(room < budget ? room : budget);
		start = P.k->start_position;
	}
	bool mine; // (a launch with nothing to generate is one block that only runs the globals below)
	int x, yl;
	if (PART == kPrimaryWindow) {
		// thread -> (sweep over the rank's rows, row of the window, column of the window) -> the ticket that has this pixel
		const uint32_t ww = win.x1 - win.x0, per = ww * (win.yl1 - win.yl0);
		const uint32_t sweep = index / per, rem = index - sweep * per, row = rem / ww;
		x = (int)(win.x0 + (rem - row * ww));
		yl = (int)(win.yl0 + row);
		const unsigned long long at = (unsigned long long)sweep * P.localPixels + (uint32_t)yl * P.W + (uint32_t)x; // = start + ticket
		mine = at >= start && at - start < nNew;
		index = (uint32_t)(at - start);
	} else if (PART == kPrimaryMapped) {
		// the ticket: budget <= total in mapped mode (tyr_set_sample_map sets it to total, launches only lower it) and index < nNew <= budget.
		// A budget above the list is a broken invariant: the rays are made from pixel 0 and the error word says so.
		mine = index < nNew;
		const bool inList = budget <= (unsigned long long)map.total;
		const uint32_t ticket = map.total - (uint32_t)budget + index;
		const uint32_t p = (mine && inList) ? map.list[ticket] : 0u;
		if (mine && !inList && index == 0u)
			atomicOr(&P.k->device_error, kErrTicketRange);
		x = (int)(p % P.W);
		yl = (int)(p / P.W);
	} else {
		x = (int)((start + index) % P.W);
		yl = (int)(((start + index) / P.W) % P.localRows);
		mine = index < nNew;
		if (PART == kPrimaryRest)
			mine = mine && !((uint32_t)x >= win.x0 && (uint32_t)x < win.x1 && (uint32_t)yl >= win.yl0 && (uint32_t)yl < win.yl1);
	}
	const uint32_t vslot = index + cnt; // the slot the serial order gives this ray (kernel.cu:254): what seeds its shading
	const int y = yl * (int)P.nranks + (int)P.rank; // nranks == 1: kernel.cu:264
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	f3 lensPoint = mk3(0.f, 0.f, 0.f), direction = mk3(0.f, 0.f, 0.f);
	float2 hitRecord = make_float2(kVeryFar, 0.f);
	bool tree = false, sky = false;
	// (the two parts: a wave none of whose lanes has a ray -- the other part's pixels -- has nothing to compute; a whole
	// top-up, raster or mapped, computes every wave)
	if (PART == kPrimaryWhole || PART == kPrimaryMapped || __ballot(mine) != 0ull) {
		uint32_t seed = camera_seed(P, index);
		const CameraRay cr = camera_lens(P, seed, camera_focus(P, seed, x, y), ld3(P.camPos), ld3(P.camRight), ld3(P.camUp));
		lensPoint = cr.origin, direction = cr.direction;

		// extend's sphere half for this ray, while it is in registers (k_extend_spheres then only has the survivors of the
		// last iteration to do), and the traversal's own first test (root_ref at the refill of k_trace_flat: same function,
		// same bound, same answer): a ray that fails it goes to class 1 and is finished with this record
		hitRecord = sphere_hit_record(P, lensPoint, direction);
		tree = mine && P.scene.rootRef != kRefDone && root_ref(P.scene, make_ray(lensPoint, direction), hitRecord.x) != kRefDone;
		// A camera ray that hits no sphere and fails the root box is finished before it is queued (P.retireSky, tyr_render's
		// merged path): what shade would do with it is fixed -- kernel.cu:613-617 with the fresh ray's lastSpecular = true and
		// direct = (1,1,1) (kernel.cu:295, variables.h:33): color = sunsky(direction), one finished path, no survivor, no shadow
		// ray, and NO random number drawn -- so it is done here, while the direction is in registers: the pixel gets its
		// radiance (the same operations: 0 + 1 * x is x), the ray's survive byte is 0, and the record is never written or read
		// (42 % of the first wavefront's rays on C3: 112 bytes of queue traffic and a shade lane each).  Every count stays: the
		// ray was generated and traced (n_live and the totals are sums, not queue lengths).
		sky = P.retireSky != 0u && mine && !tree && !(hitRecord.x < kVeryFar);
		if (__ballot(sky) != 0ull) {
			f3 radiance = mk3(0.f, 0.f, 0.f);
			if (sky) {
				if (P.sun.sunAngularDiameterCos == 1.0f) {
					radiance = mk3(1.0f, 0.0f, 0.0f); // sunsky.cu:118-119
				} else {
					const Atmosphere a = atmosphere(P.sun, direction);
					radiance = sunsky_radiance(P.sun, a);
				}
				P.survFlag[vslot] = 0; // what k_shade writes for a ray that does not survive (k_scan_words reads every slot below n_live)
			}
			accumulate_pixels_wave(P.blit, y * (int)P.W + x, radiance, sky ? 1 : 0);
		}
		if (PART == kPrimaryRest) {
			if (__ballot(tree) != 0ull) {
				if (lane == 0)
					atomicAdd(&P.k->primary_strays, (uint32_t)__popcll(__ballot(tree)));
				bool overflow = false;
				for (unsigned long long m; (m = __ballot(tree)) != 0ull;) {
					if (lane == (uint32_t)__ffsll((long long)m) - 1u) {
						hitRecord = trace_stray(kernarg_view<FrameParams>().scene, strayStack + wave * kStackSize, lensPoint, direction, hitRecord, overflow);
						tree = false; // its record carries the answer: it joins the rays that are finished with theirs
					}
				}
				if (__ballot(overflow) != 0ull && lane == 0)
					atomicOr(&P.k->device_error, kErrStackOverflow);
			}
		}
	}
	// the block's rays of either class go to segment blockIdx % 8 of that class, behind what it holds: one atomic each
	const unsigned long long bt = __ballot(tree), bsky = __ballot(mine && !tree && !sky), below = (1ull << lane) - 1ull;
	if (lane == 0) {
		cntSh[wave] = (uint32_t)__popcll(bt);
		cntSh[4 + wave] = (uint32_t)__popcll(bsky);
	}
	__syncthreads();
	uint32_t before[2] = { 0, 0 }, total[2] = { 0, 0 };
#pragma unroll
	for (uint32_t w = 0; w < kBlock / 64; ++w) {
		if (w < wave) {
			before[0] += cntSh[w];
			before[1] += cntSh[4 + w];
		}
		total[0] += cntSh[w];
		total[1] += cntSh[4 + w];
	}
	const uint32_t seg = blockIdx.x & (kSegs - 1u);
	if (threadIdx.x < kClasses) {
		const uint32_t c = threadIdx.x, n = total[c];
		uint32_t base = 0;
		if (n) {
			base = atomicAdd(&P.segWork[c * kClassWords + seg * kSegStride], n);
			if (base + n > P.segCap) {
				atomicOr(&P.k->device_error, kErrQueueOverflow);
				base = 0xffffffffu;
			}
		}
		baseSh[c] = base;
	}
	__syncthreads();
	const uint32_t cls = tree ? 0u : 1u;
	if (mine && !sky && baseSh[cls] != 0xffffffffu) {
		const uint32_t rank = before[cls] + (uint32_t)__popcll((tree ? bt : bsky) & below);
		const uint32_t slot = cls * P.classStride + seg_phys(seg, baseSh[cls] + rank);
		// kernel.cu:295: {origin, direction, {1,1,1}, 0, 0, 0, pixel}; lastSpecular defaults to true (variables.h:33)
		P.work.o_dx[slot] = make_float4(lensPoint.x, lensPoint.y, lensPoint.z, direction.x);
		P.work.dyz[slot] = make_float2(direction.y, direction.z);
		P.work.direct_ix[slot] = make_float4(1.0f, 1.0f, 1.0f, __int_as_float(y * (int)P.W + x));
		P.work.flags[slot] = 0u | (1u << 8);
		P.work.hit[slot] = hitRecord;
		P.work.key[slot] = vslot;
	}
	if (PART == kPrimaryRest)
		return; // (k_primary_window has opened the iteration)
	// set_wavefront_globals (kernel.cu:227-244, launched behind primary_rays at kernel.cu:720): by the block that finishes last
	__syncthreads();
	if (threadIdx.x == 0) {
		// eight counters (one word serves only ~88 returning atomics per microsecond; a 16.6 M-ray top-up is 65 k blocks):
		// the block that completes its word counts the word, the block that completes the eighth word is the last.
		// No fence: the last block reads nothing the others wrote, it only overwrites counts they have finished reading
		// (their own stores depended on those reads); a release here is an L2 write-back per block -- 2.4 ms of a 16.6 M-ray
		// top-up when it was tried.
		const uint32_t w = blockIdx.x & (kTicketWords - 1u);
		const uint32_t mineOfWord = (gridDim.x - w + kTicketWords - 1u) / kTicketWords; // blocks b with b % 8 == w
		uint32_t last = 0;
		if (atomicAdd(&P.k->primary_done[w * 32], 1u) + 1u == mineOfWord) {
			const uint32_t words = gridDim.x < kTicketWords ? gridDim.x : kTicketWords;
			last = atomicAdd(&P.k->primary_blocks_done, 1u) + 1u == words ? 1u : 0u;
		}
		if (PART == kPrimaryWindow && last) {
			// the top-up, for k_primary_rest: what every block of this launch computed from the counts the globals now overwrite
			P.k->plan_cnt = cnt;
			P.k->plan_new = nNew;
			P.k->plan_start = start;
		}
		lastSh = last;
	}
	__syncthreads();
	if (lastSh)
		wavefront_globals(P);
}

__global__ void __launch_bounds__(kBlock) k_primary(const FrameParams P) { primary_rays<kPrimaryWhole>(P, PrimaryWindow{}); }
__global__ void __launch_bounds__(kBlock) k_primary_window(const FrameParams P, const PrimaryWindow win) { primary_rays<kPrimaryWindow>(P, win); }
__global__ void __launch_bounds__(kBlock) k_primary_rest(const FrameParams P, const PrimaryWindow win) { primary_rays<kPrimaryRest>(P, win); }
__global__ void __launch_bounds__(kBlock) k_primary_mapped(const FrameParams P, const MappedPrimary map) { primary_rays<kPrimaryMapped>(P, PrimaryWindow{}, map); }

// extend pre-pass: kernel.cu:125-136 (spheres first; their distance bounds the BVH search)
// (grid-stride over the device's count: the host may have sized the grid from an upper bound, and a capped grid makes a
// loose bound free)
__global__ void __launch_bounds__(kBlock) k_extend_spheres(const FrameParams P) {
	// the counts once per block through LDS: 32 loads of eight hot cache lines per THREAD were a fixed ~25 us of this kernel
	__shared__ uint32_t cntSh[2 * kClasses * kSegs];
	if (threadIdx.x < kClasses * kSegs) {
		const uint32_t c = threadIdx.x / kSegs, w = threadIdx.x % kSegs;
		cntSh[threadIdx.x] = P.k->segSurv[c][w];
		cntSh[kClasses * kSegs + threadIdx.x] = P.segWork[c * kClassWords + w * kSegStride];
	}
	__syncthreads();
	const uint32_t first = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
	// the survivors of the last iteration, both classes: the records in front of what a top-up appended (k_primary has done
	// its own rays).  Class 0: the distance bounds the BVH search; class 1: the record is the ray's answer.
	// (validity straight from the LDS table, one read per test: a private array of the eight counts is "promoted" to LDS
	// by the compiler anyway -- 64 bytes per thread -- and then read eight times per test)
	auto extent_of = [&](uint32_t at) {
		uint32_t m = 0;
#pragma unroll
		for (uint32_t w = 0; w < kSegs; ++w)
			m = cntSh[at + w] > m ? cntSh[at + w] : m;
		return ((m + 63u) >> 6) * (kSegs * 64u);
	};
	auto holds = [&](uint32_t at, uint32_t j) { return (((j >> 9) << 6) | (j & 63u)) < cntSh[at + ((j >> 6) & (kSegs - 1u))]; };
	for (uint32_t c = 0; c < kClasses; ++c) {
		const uint32_t surv = c * kSegs, now = (kClasses + c) * kSegs;
		// class 0 is walked up to its extent: the slots at the segments' ends that hold no record become rays that enter
		// nothing (k_trace_flat hands out slots [0, extent) without asking)
		const uint32_t n = c == 0 ? extent_of(now) : extent_of(surv), base = c * P.classStride;
		for (uint32_t j = first; j < n; j += stride) {
			const uint32_t slot = base + j;
			if (!holds(surv, j)) {
				if (c == 0 && !holds(now, j))
					write_dead_ray(P.work, slot);
				continue;
			}
			const float4 a = P.work.o_dx[slot];
			const float2 b = P.work.dyz[slot];
			P.work.hit[slot] = sphere_hit_record(P, mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y));
		}
	}
}

// The same for an iteration whose sphere pre-pass does not run (no survivors: a render's first wavefront): the slots at
// the ends of the eight segments that hold no record become rays that enter nothing.  Block w does segment w; what == 0:
// class 0 of the work queue, 1: the shadow queue (unused: its pre-pass always runs).
__global__ void __launch_bounds__(kBlock) k_pad_holes(const FrameParams P, uint32_t workQueue, uint32_t shadowQueue, uint32_t resetTickets) {
	const uint32_t w = blockIdx.x & (kSegs - 1u), what = blockIdx.x / kSegs;
	if (resetTickets && blockIdx.x == 0 && threadIdx.x < kTicketWords)
		P.k->extend_chunks[threadIdx.x * 32] = 0; // k_trace_flat's tickets, when no connect pre-pass opens the launch that ends a render (P.foldSpheres)
	if ((what == 0 && !workQueue) || (what == 1 && !shadowQueue))
		return;
	const uint32_t* cnt = what == 0 ? P.segWork : P.kc->seg;
	const uint32_t mine = cnt[w * kSegStride], ext = queue_extent(cnt) / kSegs; // records per segment up to the extent
	for (uint32_t j = mine + threadIdx.x; j < ext; j += kBlock) {
		const uint32_t slot = seg_phys(w, j);
		if (what == 0)
			write_dead_ray(P.work, slot);
		else
			reinterpret_cast<float*>(&P.shadow.color[slot])[3] = 1.0f;
	}
}

// the counter words the host changes between stages (kernels.hpp "CounterPoke"): one block, plain stores -- the launch is alone on the stream
__global__ void __launch_bounds__(kBlock) k_poke_counters(DevCounters* __restrict__ k, const CounterPoke p) {
	if (p.what & kPokeResetQueue) {
		uint32_t* const seg = &k->seg[p.queue & 1u][0][0];
		for (uint32_t i = threadIdx.x; i < kClasses * kSegs * kSegStride; i += kBlock)
			seg[i] = 0u;
		if (threadIdx.x < kClasses * kSegs)
			(&k->segSurv[0][0])[threadIdx.x] = 0u;
		if (threadIdx.x == 0)
			k->primary_ray_cnt = 0u;
	}
	if (threadIdx.x == 0) {
		if (p.what & kPokeBudget)
			k->budget_remaining = p.budget;
		if (p.what & kPokeLiveShadow) {
			k->n_live = p.nLive;
			k->shadow_ray_cnt = p.shadows;
		}
	}
}

// connect pre-pass: the sphere half of intersect_scene_simple (kernel.cu:168-172).  Any-hit does not
// depend on test order, so spheres go first and an occluded ray never enters the BVH.
// color.w (unused by the reference's 44-byte record) carries the flag.
__global__ void __launch_bounds__(kBlock) k_connect_spheres(const FrameParams P) {
	const uint32_t first = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
	if (first < kTicketWords)
		P.k->extend_chunks[first * 32] = 0; // k_trace_flat's tickets, when this pre-pass opens the launch that ends a render (no set_wavefront_globals in front of it)
	__shared__ uint32_t cntSh[kSegs];
	if (threadIdx.x < kSegs)
		cntSh[threadIdx.x] = P.kc->seg[threadIdx.x * kSegStride];
	__syncthreads();
	uint32_t m = 0;
#pragma unroll
	for (uint32_t w = 0; w < kSegs; ++w)
		m = cntSh[w] > m ? cntSh[w] : m;
	const uint32_t n = ((m + 63u) >> 6) * (kSegs * 64u);
	for (uint32_t index = first; index < n; index += stride) {
		if ((((index >> 9) << 6) | (index & 63u)) >= cntSh[(index >> 6) & (kSegs - 1u)]) {
			reinterpret_cast<float*>(&P.shadow.color[index])[3] = 1.0f; // a hole at a segment's end: "occluded" retires it at the traversal's refill
			continue;
		}
		const float4 a = P.shadow.o_dx[index];
		const float4 b = P.shadow.dyz_cd_ix[index];
		const f3 o = mk3(a.x, a.y, a.z), d = mk3(a.w, b.x, b.y);
		const float closest = b.z;
		bool occluded = false;
#pragma unroll
		for (int i = TYR_NUM_SPHERES; i--;) {
			const float t = sphere_intersect(P.spheres[i], o, d);
			occluded = occluded || (t && (t + kEpsilon) < closest);
		}
		reinterpret_cast<float*>(&P.shadow.color[index])[3] = occluded ? 1.0f : 0.0f;
	}
}

// ======================================================================================
// The serial order, recovered as numbers (kernels.hpp "Queues"): shade wrote one byte per ray at its virtual slot --
// survived or not; rank(v) = survivors below v is the survivor's slot in the next iteration by the reference's serial
// ticket order (kernel.cu:607 with the atomics in slot order).  k_scan_words packs 64 bytes into one word and scans the
// words' counts inside 16384-slot blocks; the block that finishes last scans the blocks' totals.  v_lookup() adds the three parts.
// ======================================================================================
constexpr uint32_t kScanBlockSlots = 64u * kBlock;
__global__ void __launch_bounds__(kBlock) k_scan_words(const FrameParams P) {
	__shared__ uint32_t waveSum[kBlock / 64];
	const uint32_t n = *P.scanLive; // &k->n_live
	const uint32_t e = blockIdx.x * kBlock + threadIdx.x, first = e * 64u;
	if (blockIdx.x * kScanBlockSlots >= n)
		return; // (the whole block: the host sized the grid from an upper bound.  With n == 0 that is EVERY block, block 0 and the fold below
		        // included: an iteration without rays opens no successor -- k_shade's shadeOpensNext agrees, host/driver.cpp render_run_ahead
		        // states the invariant: nothing is ever queued behind an empty iteration)
	unsigned long long word = 0ull;
	if (first < n) {
		uint4* p = reinterpret_cast<uint4*>(P.survFlag + first);
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const uint4 q = p[k];
			// read and -- when this iteration's shade finished survivors in place (P.retireGhosts) -- cleared: such a survivor occupies
			// a slot of the NEXT iteration's order that nobody will write, and it must read "did not survive" there.  (Every other
			// slot below the next iteration's ray count is written by whoever makes or shades its ray.)
			if (P.retireGhosts)
				p[k] = make_uint4(0u, 0u, 0u, 0u);
			const uint32_t x[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
			for (int j = 0; j < 4; ++j) { // four bytes, each 0 or 1 -> four bits
				const uint32_t b = (x[j] & 1u) | ((x[j] >> 7) & 2u) | ((x[j] >> 14) & 4u) | ((x[j] >> 21) & 8u);
				word |= (unsigned long long)b << (16 * k + 4 * j);
			}
		}
		if (n - first < 64u)
			word &= (1ull << (n - first)) - 1ull; // bytes past the queue's end were never written
	}
	const uint32_t c = (uint32_t)__popcll(word);
	uint32_t incl = c;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t v = __shfl_up(incl, o, 64);
		if (lane >= (uint32_t)o)
			incl += v;
	}
	if (lane == 63u)
		waveSum[wave] = incl;
	__syncthreads();
	uint32_t before = 0, total = 0;
#pragma unroll
	for (uint32_t w = 0; w < kBlock / 64; ++w) {
		if (w < wave)
			before += waveSum[w];
		total += waveSum[w];
	}
	P.vWordOut[e] = word;
	P.vPreOut[e] = before + incl - c;
	// the blocks' totals become exclusive prefixes in the block that finishes last
	__shared__ uint32_t lastSh, carrySh;
	if (threadIdx.x == 0) {
		__hip_atomic_store(&P.vBlkOut[blockIdx.x], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		__asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the total has arrived before this block counts as done (no L2 write-back: see k_shade)
		const uint32_t nBlocksLive = (n + kScanBlockSlots - 1) / kScanBlockSlots;
		lastSh = atomicAdd(&P.k->scan_blocks_done, 1u) + 1u == nBlocksLive ? 1u : 0u;
		carrySh = 0;
	}
	__syncthreads();
	if (!lastSh)
		return;
	const uint32_t nBlocks = (n + kScanBlockSlots - 1) / kScanBlockSlots;
	for (uint32_t base = 0; base < nBlocks; base += kBlock) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < nBlocks ? __hip_atomic_load(&P.vBlkOut[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
		uint32_t inc2 = v;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t u = __shfl_up(inc2, o, 64);
			if (lane >= (uint32_t)o)
				inc2 += u;
		}
		__syncthreads(); // waveSum is reused
		if (lane == 63u)
			waveSum[wave] = inc2;
		__syncthreads();
		uint32_t before2 = carrySh, total2 = 0;
#pragma unroll
		for (uint32_t w = 0; w < kBlock / 64; ++w) {
			if (w < wave)
				before2 += waveSum[w];
			total2 += waveSum[w];
		}
		if (i < nBlocks)
			P.vBlkOut[i] = before2 + inc2 - v;
		__syncthreads();
		if (threadIdx.x == 0)
			carrySh += total2;
		__syncthreads();
	}
	// the counter is left as the next scan expects it.  (set_wavefront_globals zeroes it too -- but a scan done by the next traversal launch,
	// TYR_TUNE_SCAN_IN_TRACE, runs BEHIND the next iteration's set_wavefront_globals, and the scan after it may be this kernel's)
	if (threadIdx.x == 0)
		P.k->scan_blocks_done = 0;
	// P.foldNextPrologue (tyr_render, an iteration whose successor is already being queued and cannot top the queue up: the budget
	// is spent): what would open that successor -- a one-block k_primary launch for set_wavefront_globals (kernel.cu:227-244) and
	// k_pad_holes in front of its traversal launch, two launches and two gaps between dependent kernels (~25 us of a ~550 us thin
	// iteration) -- is done here, by the block that ends this iteration's last kernel.  Everything it reads is final (shade's
	// launch has ended), everything it resets has been consumed (this iteration's work queue, the other set of shadow counters).
	if (P.foldNextPrologue) {
		pad_work_holes_block(P.next, P.segNext);   // the successor's work queue: class 0's segment ends
		pad_shadow_holes_block(P.shadow, P.kc->seg); // ... and the shadow rays it carries
		__syncthreads();
		wavefront_globals_for(P, P.segWork, P.kcPrev);
	}
}


// ======================================================================================
// blit_onto_framebuffer, kernel.cu:648-662 -> linear RGBA32F
// ======================================================================================
__global__ void __launch_bounds__(kBlock) k_resolve(const float4* __restrict__ blit, float4* __restrict__ out, uint32_t nPixels) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= nPixels)
		return;
	const float4 color = blit[i];
	const float r = color.x / color.w, g = color.y / color.w, b = color.z / color.w;
	constexpr float inv_gamma = 1.0f / 2.2f;
	out[i] = make_float4(dm::powf_det(r / (r + 1.f), inv_gamma), dm::powf_det(g / (g + 1.f), inv_gamma), dm::powf_det(b / (b + 1.f), inv_gamma),
		dm::powf_det(1.f / (1.f + 1.f), inv_gamma));
}

// ======================================================================================
// tyr_vecmath_probe: hip/vecmath.hpp (and the deterministic pow / exp) evaluated ON THE DEVICE over arrays, so that the
// functions every kernel is built from can be pinned to the vendored glm's answers (tests/golden/ref_glm.npz).
// Ops 0-19: the op codes of oracle/ref_harness.cpp ref_glm.
// ======================================================================================
// Ops >= 32 are the project's own (no glm counterpart): the numeric contract's functions (hip/detmath.hpp) with the binary64
// values they round, and the samplers of device_common.hpp, against the oracle's orc_dm_map / orc_sampler_map (DESIGN.md
// section 2).  Three 32-bit WORDS per element, so that binary64 values (low word first) and seeds pass as bit patterns.  Each
// op restates the function's own lines with the function's own building blocks; a value the function does not reach for this
// argument (an early return) is 0.
__device__ __forceinline__ void put64(uint32_t* w, double v) {
	const unsigned long long u = (unsigned long long)__double_as_longlong(v);
	w[1] = (uint32_t)u;
	w[2] = (uint32_t)(u >> 32);
}
__device__ void contract_probe(int op, f3 A, f3 B, uint32_t seedWord, uint32_t* __restrict__ w) {
	const float x = A.x;
	w[0] = w[1] = w[2] = 0u;
	switch (op) {
	case 32:   // sinf_det: [result, r]
	case 33:   //           [q, the binary64 value that is rounded]
	case 34:   // cosf_det: [result, r]
	case 35: { //           [q, the binary64 value that is rounded]
		const bool isSin = op < 34;
		if (!(op & 1))
			w[0] = __float_as_uint(isSin ? dm::sinf_det(x) : dm::cosf_det(x));
		if (!(fabsf(x) < 1048576.0f))
			break;
		int q;
		const double r = dm::reduce_pio2((double)x, q);
		if (!(op & 1)) {
			put64(w, r);
			break;
		}
		w[0] = (uint32_t)q;
		if (isSin) {
			const double s = (q & 1) ? dm::cos_poly(r) : dm::sin_poly(r);
			put64(w, (q & 2) ? -s : s);
		} else {
			const double c = (q & 1) ? dm::sin_poly(r) : dm::cos_poly(r);
			put64(w, ((q + 1) & 2) ? -c : c);
		}
		break;
	}
	case 36: { // sincosf_det: [sin, cos, 0]
		float s, c;
		dm::sincosf_det(x, s, c);
		w[0] = __float_as_uint(s);
		w[1] = __float_as_uint(c);
		break;
	}
	case 37:   // expf_det: [result, kd]
	case 38:   //           [0, r]
	case 39: { //           [0, exp_poly(r) * pow2i(kd)]
		if (op == 37)
			w[0] = __float_as_uint(dm::expf_det(x));
		const double xd = (double)x;
		if (x != x || xd > 89.0 || xd < -104.0)
			break;
		const double kd = dm::rne(xd * dm::kLog2e);
		const double r = (xd - kd * dm::kLn2Hi) - kd * dm::kLn2Lo;
		put64(w, op == 37 ? kd : op == 38 ? r : dm::exp_poly(r) * dm::pow2i((int)kd));
		break;
	}
	case 40:   // powf_det(A.x, B.x): [result, log2_det(x)]
	case 41:   //                     [0, t]
	case 42:   //                     [0, w]
	case 43: { //                     [0, exp_poly(w) * pow2i(kd)]
		const float y = B.x;
		if (op == 40)
			w[0] = __float_as_uint(dm::powf_det(x, y));
		if (y != y || !(x > 0.0f) || x == __builtin_inff())
			break;
		const double l2 = dm::log2_det((double)x);
		const double t = (double)y * l2;
		if (op <= 41) {
			put64(w, op == 40 ? l2 : t);
			break;
		}
		if (t > 129.0 || t < -152.0)
			break;
		const double kd = dm::rne(t);
		const double ww = (t - kd) * dm::kLn2;
		put64(w, op == 42 ? ww : dm::exp_poly(ww) * dm::pow2i((int)kd));
		break;
	}
	case 44: { // seed = the word at A.x: [rng_float, seed after, rng_int_0_max(16) from the same seed]
		uint32_t s = seedWord, s2 = s;
		w[0] = __float_as_uint(rng_float(s));
		w[1] = s;
		w[2] = (uint32_t)rng_int_0_max(s2, 16);
		break;
	}
	case 45: { // [rng_float2, seed after, seed after rng_int_0_max(16)]
		uint32_t s = seedWord, s2 = s;
		w[0] = __float_as_uint(rng_float2(s));
		w[1] = s;
		(void)rng_int_0_max(s2, 16);
		w[2] = s2;
		break;
	}
	case 46: { // stratified_sample: [sx, sy, seed after]
		uint32_t s = seedWord;
		float sx, sy;
		stratified_sample(s, sx, sy);
		w[0] = __float_as_uint(sx);
		w[1] = __float_as_uint(sy);
		w[2] = s;
		break;
	}
	case 47: { // concentric_sample_disk(A.x, A.y): [dx, dy, 0]
		float dx, dy;
		concentric_sample_disk(A.x, A.y, dx, dy);
		w[0] = __float_as_uint(dx);
		w[1] = __float_as_uint(dy);
		break;
	}
	case 48:   // orthonormal_basis_naive(A): u
	case 49: { //                             v
		f3 u, v;
		orthonormal_basis_naive(A, u, v);
		const f3 r = op == 48 ? u : v;
		w[0] = __float_as_uint(r.x);
		w[1] = __float_as_uint(r.y);
		w[2] = __float_as_uint(r.z);
		break;
	}
	// the winding numbers' binary64 building blocks (include/tyr_c.h "Winding numbers"): [0, value]
	case 50: put64(w, dm::atan2_det((double)x, (double)B.x)); break;
	case 51: put64(w, (double)x / (double)B.x); break;
	case 52: put64(w, __builtin_sqrt((double)x * (double)B.x)); break;
	default: break;
	}
}

__global__ void __launch_bounds__(kBlock) k_vecmath_probe(int op, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, uint32_t n, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n)
		return;
	const f3 A = ld3(a + 3 * i), B = ld3(b + 3 * i), Cc = ld3(c + 3 * i);
	if (op >= 32) {
		contract_probe(op, A, B, reinterpret_cast<const uint32_t*>(a)[3 * i], reinterpret_cast<uint32_t*>(out) + 3 * i);
		return;
	}
	f3 r = mk3(0.f, 0.f, 0.f);
	switch (op) {
	case 0: r.x = dot(A, B); break;
	case 1: r = cross(A, B); break;
	case 2: r = normalize(A); break;
	case 3: r.x = length(A); break;
	case 4: r = reflect(A, B); break;
	case 5: r = mk3(gmin(A.x, B.x), gmin(A.y, B.y), gmin(A.z, B.z)); break;
	case 6: r = mk3(gmax(A.x, B.x), gmax(A.y, B.y), gmax(A.z, B.z)); break;
	case 7: r = mk3(gclamp(A.x, B.x, B.y), gclamp(A.y, B.x, B.y), gclamp(A.z, B.x, B.y)); break;
	case 8: r = gmix(A, B, Cc.x); break;
	case 9: r.x = gsmoothstep(Cc.x, Cc.y, A.x); break;
	case 10: // exponent 0.5 is the path's closed form sqrt (sunsky.hpp: pow(inscatter * Fex, vec3(0.5)), sunsky.cu:66)
		r = mk3(B.x == 0.5f ? sqrtf(A.x) : dm::powf_det(A.x, B.x), B.y == 0.5f ? sqrtf(A.y) : dm::powf_det(A.y, B.y), B.z == 0.5f ? sqrtf(A.z) : dm::powf_det(A.z, B.z));
		break;
	case 11: r = A / Cc.x; break;
	case 12: r = A * Cc.x; break;
	case 13: r = Cc.x * A; break;
	case 14: r = mk3(dm::expf_det(A.x), dm::expf_det(A.y), dm::expf_det(A.z)); break;
	case 15: r = A * B; break;
	case 16: r = A / B; break;
	case 17: r = -A; break;
	case 18: r = A + B; break;
	case 19: r = A - B; break;
	default: break;
	}
	out[3 * i + 0] = r.x;
	out[3 * i + 1] = r.y;
	out[3 * i + 2] = r.z;
}

// ======================================================================================
// tyr_sunsky_probe: sun / sky / sunsky and the sun-cone sample exactly as k_shade evaluates them (one shared
// atmosphere() block, then the radiance the ray asked for; shade.hip "The atmosphere ..."), over arrays, so that the
// device arithmetic can be pinned to the reference's own sunsky.cu (tests/golden/ref_sunsky.npz).
// ======================================================================================
__global__ void __launch_bounds__(kBlock) k_sunsky_probe(const SunParams S, int which, const float* __restrict__ dirs, uint32_t n, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (which == 3) { // one stream, serial by definition: thread 0 draws the n samples in order
		if (i != 0)
			return;
		uint32_t seed = __float_as_uint(dirs[0]);
		for (uint32_t j = 0; j < n; ++j) {
			const f3 r = cone_sample(S, seed);
			out[3 * j + 0] = r.x;
			out[3 * j + 1] = r.y;
			out[3 * j + 2] = r.z;
		}
		out[3 * n] = __uint_as_float(seed);
		return;
	}
	if (i >= n)
		return;
	const f3 viewDir = ld3(dirs + 3 * i);
	f3 r;
	if (which == 2 && S.sunAngularDiameterCos == 1.0f) {
		r = mk3(1.0f, 0.0f, 0.0f); // sunsky.cu:118-119
	} else {
		const Atmosphere a = atmosphere(S, viewDir);
		r = which == 0 ? sun_radiance(S, a) : which == 1 ? sky_radiance(a) : sunsky_radiance(S, a);
	}
	out[3 * i + 0] = r.x;
	out[3 * i + 1] = r.y;
	out[3 * i + 2] = r.z;
}

// ======================================================================================
// extend_debug_BVH, kernel.cu:300-328 via intersect_scene_DEBUG (143-160) and CachedBVH::intersect_debug (bvh.h:164-209):
// the reference's compile-time BVH_DEBUG picture of the traversal cost.  One thread per slot on the pair nodes with the
// reference's counting rule (traversals = nodes visited - 1); a diagnostic, not a hot path.
// ======================================================================================
__global__ void __launch_bounds__(kBlock) k_extend_debug(const FrameParams P) {
	uint32_t refs[kStackSize];
	float ts[kStackSize];
	TravStack st;
	st.bind(refs, ts);
	st.reset();
	uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
	{
		const uint32_t c = slot >= P.classStride ? 1u : 0u, j = slot - c * P.classStride;
		const uint32_t* cnt = P.segWork + c * kClassWords;
		if (c >= kClasses || j >= queue_extent(cnt) || !slot_valid(cnt, j))
			return;
	}
	const float4 a = P.work.o_dx[slot];
	const float2 b = P.work.dyz[slot];
	float dist = kVeryFar; // kernel.cu:145; the spheres are commented out there (147-155)
	int prim = 0, traversals = 0;
	if (P.scene.rootRef != kRefDone) {
		VisitCount vc{ 0, 0 };
		const RayConst r = make_ray(mk3(a.x, a.y, a.z), mk3(a.w, b.x, b.y));
		const bool hit = bvh_closest(P.scene, r, dist, prim, st, vc);
		traversals = (int)vc.nodes - 1; // bvh.h:172-175: the counter starts at -1 and counts loop iterations
		P.work.hit[slot] = make_float2(dist, __uint_as_float(hit ? (uint32_t)prim : 0u));
		if (st.overflow)
			atomicOr(&P.k->device_error, kErrStackOverflow);
	} else {
		P.work.hit[slot] = make_float2(dist, 0.0f);
	}
	float* px = reinterpret_cast<float*>(&P.blit[__float_as_int(P.work.direct_ix[slot].w)]);
	int green = (int)((0.0002f * (float)traversals) * 255.99f);
	green = green > 255 ? 255 : green;
	px[1] = (float)green;
	px[3] = 1.0f;
	if (traversals >= 70) { // "Color very costly regions distinctly"
		px[0] = (float)green;
		px[1] = 0.0f;
	}
}

// ---- launch wrappers ---------------------------------------------------------------------

constexpr uint32_t kPrepassMaxBlocks = 8192; // 8 waves of 256 threads per SIMD of a 256-CU part: enough to stream at full rate
StageEvents*& open_stage_events() {
	static thread_local StageEvents* open = nullptr;
	return open;
}
void launch_poke_counters(DevCounters* k, const CounterPoke& p, hipStream_t stream) {
	hipLaunchKernelGGL(k_poke_counters, dim3(1), dim3(kBlock), 0, stream, k, p);
}
void launch_pad_holes(const FrameParams& P, bool workQueue, bool shadowQueue, hipStream_t stream, bool resetTickets) {
	launch_in_stage(k_pad_holes, dim3(2 * kSegs), dim3(kBlock), stream, P, workQueue ? 1u : 0u, shadowQueue ? 1u : 0u, resetTickets ? 1u : 0u);
}
void launch_primary(const FrameParams& P, uint32_t maxNew, hipStream_t stream) {
	// always launched: its last block is set_wavefront_globals
	launch_in_stage(k_primary, dim3(maxNew ? blocks_for(maxNew) : 1u), dim3(kBlock), stream, P);
}
void launch_primary_mapped(const FrameParams& P, const MappedPrimary& map, uint32_t maxNew, hipStream_t stream) {
	// always launched: its last block is set_wavefront_globals
	launch_in_stage(k_primary_mapped, dim3(maxNew ? blocks_for(maxNew) : 1u), dim3(kBlock), stream, P, map);
}
void launch_primary_window(const FrameParams& P, const PrimaryWindow& win, uint32_t maxNew, hipStream_t stream) {
	// the sweeps over the rank's rows that maxNew tickets can touch from any start position, each with the window's pixels
	const unsigned long long per = (unsigned long long)(win.x1 - win.x0) * (win.yl1 - win.yl0);
	const unsigned long long sweeps = maxNew ? ((unsigned long long)P.localPixels + maxNew - 2ull) / P.localPixels + 1ull : 0ull;
	const unsigned long long threads = per * sweeps;
	launch_in_stage(k_primary_window, dim3(threads ? (uint32_t)((threads + kBlock - 1) / kBlock) : 1u), dim3(kBlock), stream, P, win);
}
void launch_primary_rest(const FrameParams& P, const PrimaryWindow& win, uint32_t maxNew, hipStream_t stream, hipEvent_t stop) {
	if (stop)
		hipExtLaunchKernelGGL(k_primary_rest, dim3(blocks_for(maxNew)), dim3(kBlock), 0, stream, nullptr, stop, 0, P, win);
	else
		hipLaunchKernelGGL(k_primary_rest, dim3(blocks_for(maxNew)), dim3(kBlock), 0, stream, P, win);
}
void launch_scan(const FrameParams& P, uint32_t maxLive, hipStream_t stream) {
	if (maxLive == 0)
		return;
	launch_in_stage(k_scan_words, dim3((maxLive + kScanBlockSlots - 1) / kScanBlockSlots), dim3(kBlock), stream, P);
}
void launch_vecmath_probe(int op, const float* a, const float* b, const float* c, uint32_t n, float* out, hipStream_t stream) {
	hipLaunchKernelGGL(k_vecmath_probe, dim3(blocks_for(n ? n : 1)), dim3(kBlock), 0, stream, op, a, b, c, n, out);
}
void launch_sunsky_probe(const SunParams& S, int which, const float* dirs, uint32_t n, float* out, hipStream_t stream) {
	hipLaunchKernelGGL(k_sunsky_probe, dim3(blocks_for(which == 3 ? 1 : n)), dim3(kBlock), 0, stream, S, which, dirs, n, out);
}
void launch_extend_debug(const FrameParams& P, uint32_t maxLive, hipStream_t stream) {
	if (maxLive != 0)
		launch_in_stage(k_extend_debug, dim3(blocks_for(maxLive)), dim3(kBlock), stream, P);
}
void launch_extend_spheres(const FrameParams& P, uint32_t nSurvivors, hipStream_t stream, uint32_t maxLive) {
	// the grid also covers the hole padding at the ends of class 0's segments, which walks up to the extent of ALL this
	// iteration's rays: a handful of survivors in front of a full top-up must not leave that walk to a single block
	const uint32_t walk = std::max(nSurvivors, maxLive);
	if (nSurvivors != 0)
		launch_in_stage(k_extend_spheres, dim3(std::min(blocks_for(walk), kPrepassMaxBlocks)), dim3(kBlock), stream, P);
}
void launch_connect_spheres(const FrameParams& P, uint32_t maxShadow, hipStream_t stream) {
	launch_in_stage(k_connect_spheres, dim3(std::min(blocks_for(maxShadow), kPrepassMaxBlocks)), dim3(kBlock), stream, P);
}
void launch_resolve(const float4* blit, float4* out, uint32_t nPixels, hipStream_t stream) {
	launch_in_stage(k_resolve, dim3(blocks_for(nPixels)), dim3(kBlock), stream, blit, out, nPixels);
}

} // namespace tyr
