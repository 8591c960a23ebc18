// adaptive.cpp -- adaptive sampling behind the C ABI (include/tyr_c.h "Adaptive sampling"; the kernels are hip/adaptive.hip):
// tyr_set_sample_map builds a sample map's ticket list and enters mapped mode, tyr_allocate_samples turns an error estimate into
// a sample map.  (tyr_render_adaptive is tyr_render's loop: host/render_loop.cpp.)
#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

#include "../hip/adaptive.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

uint32_t tiles_of(uint32_t n) { return (n + kCompactTile - 1) / kCompactTile; }

// `s` behind everything queued on `from` so far
int stream_after(hipStream_t s, hipStream_t from) {
	if (from == s)
		return TYR_OK;
	hipEvent_t ready = nullptr;
	HIPCHK(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
	const hipError_t e1 = hipEventRecord(ready, from);
	const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(s, ready, 0) : e1;
	(void)hipEventDestroy(ready);
	HIPCHK(e2);
	return TYR_OK;
}

} // namespace

namespace tyr {
namespace drv {

void adaptive_free(tyr_ctx* c) {
	dev_free(c->dTickets);
	dev_free(c->dMapScratch);
	c->ticketCap = 0;
	c->ticketTotal = 0;
	c->mapped = false;
}

} // namespace drv
} // namespace tyr

extern "C" {

int tyr_set_sample_map(tyr_ctx* c, const uint32_t* spp_map, void* stream, uint64_t* total_out) {
	if (!c || !spp_map)
		return TYR_ERR_INVALID;
	int rc = use_device(c);
	if (rc)
		return rc;
	const uint32_t P = c->localPixels;
	const size_t summaryWords = kMapSummaryWords + kMaxSpp + 1u;
	// scratch: the summary + histogram first -- T is added with 64-bit atomics, so it sits at the allocation's start, 8-byte
	// aligned whatever P is -- then the map at the local pixels, then the compaction's block counts
	if (!c->dMapScratch && (rc = dev_alloc(c->dMapScratch, summaryWords + P + tiles_of(P))))
		return rc;
	uint32_t* summary = c->dMapScratch;
	uint32_t* counts = summary + summaryWords;
	uint32_t* blockCnt = counts + P;
	const hipStream_t s = c->stream;
	if ((rc = stream_after(s, stream ? static_cast<hipStream_t>(stream) : s)))
		return rc;
	HIPCHK(hipMemsetAsync(summary, 0, summaryWords * sizeof(uint32_t), s));
	SampleMapArgs A{};
	A.map = spp_map;
	A.W = c->cfg.width;
	A.localRows = c->localRows;
	A.rank = c->cfg.rank;
	A.nranks = c->cfg.nranks;
	A.counts = counts;
	A.summary = summary;
	launch_map_hist(A, P, s);
	HIPCHK(hipGetLastError());
	std::vector<uint32_t> h(summaryWords);
	HIPCHK(hipMemcpyAsync(h.data(), summary, summaryWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s)); // (from here on the caller's map is not read again)
	const uint64_t T = static_cast<uint64_t>(h[0]) | (static_cast<uint64_t>(h[1]) << 32);
	const uint32_t maxSpp = h[2];
	const uint32_t* hist = h.data() + kMapSummaryWords;
	if (h[3] != 0u || T >= (1ull << 32))
		return TYR_ERR_INVALID;
	// pass s holds the pixels with a count above s: len[s] = sum of hist[v] over v > s; off[s] = where it starts in L
	std::vector<uint32_t> len(maxSpp);
	std::vector<uint64_t> off(maxSpp + 1u, 0u);
	uint64_t running = 0;
	for (uint32_t s1 = maxSpp; s1-- > 0;) {
		running += hist[s1 + 1u];
		len[s1] = static_cast<uint32_t>(running);
	}
	for (uint32_t s1 = 0; s1 < maxSpp; ++s1)
		off[s1 + 1u] = off[s1] + len[s1];
	if (off[maxSpp] != T)
		return TYR_ERR_DEVICE; // (the histogram and the sum disagree: cannot happen)
	if (T > c->ticketCap) {
		uint32_t* grown = nullptr;
		if ((rc = dev_alloc(grown, T)))
			return rc;
		dev_free(c->dTickets); // (the stream is idle: no launch of an earlier map's list is in flight)
		c->dTickets = grown;
		c->ticketCap = T;
	}
	const uint32_t total = static_cast<uint32_t>(T);
	uint32_t* L = c->dTickets;
	if (maxSpp != 0u) {
		launch_pass_compact(nullptr, P, counts, 0u, L, total, blockCnt, s);
		uint32_t src = 0; // where the content of pass s - 1 is
		for (uint32_t s1 = 1; s1 < maxSpp;) {
			const uint32_t n = len[s1 - 1u], at = static_cast<uint32_t>(off[s1]);
			if (n < kCompactTile) { // the rest in one block, whatever the number of passes
				launch_pass_tail(L, L + src, n, counts, s1, maxSpp, at, total, s);
				break;
			}
			if (hist[s1] == 0u) { // no count ends at s1: passes s1 .. e - 1 repeat pass s1 - 1
				uint32_t e = s1 + 1u;
				while (e < maxSpp && hist[e] == 0u)
					++e;
				launch_pass_repeat(L, src, n, at, e - s1, total, s);
				s1 = e;
				continue;
			}
			launch_pass_compact(L + src, n, counts, s1, L + at, total - at, blockCnt, s);
			src = at;
			++s1;
		}
		HIPCHK(hipGetLastError());
	}
	// enter mapped mode: budget_remaining = T (tyr_set_budget's path, which the stream being idle behind the build makes exact)
	if ((rc = sync_counters(c)))
		return rc;
	c->hK->budget_remaining = T;
	if ((rc = push_counters(c)))
		return rc;
	c->ticketTotal = total;
	c->mapped = true;
	if (total_out)
		*total_out = T;
	return TYR_OK;
}

int tyr_allocate_samples(tyr_ctx* c, const float* error, const tyr_allocate_params* params, uint32_t* spp_map_out, uint64_t* total_out, void* stream) {
	if (!c || !error || !params || !spp_map_out)
		return TYR_ERR_INVALID;
	const tyr_allocate_params p = *params;
	if (p.min_spp > p.max_spp || p.max_spp < 1u || p.max_spp > kMaxSpp || p.total >= (1ull << 32))
		return TYR_ERR_INVALID;
	FilterLaunch L;
	if (int rc = L.open(c, c->alloc, stream))
		return rc;
	const hipStream_t s = L.s;
	const uint32_t P = c->localPixels, tiles = tiles_of(P);
	// scratch: the per-block scans (8 bytes per pixel), the blocks' totals, the largest error's bits and the map's sum
	if (int rc = L.buffer(c->dAllocScratch, static_cast<size_t>(P) + tiles + 2u))
		return rc;
	unsigned long long* words = c->dAllocScratch + P + tiles;
	HIPCHK(hipMemsetAsync(words, 0, 2 * sizeof(unsigned long long), s));
	const uint64_t floorTotal = static_cast<uint64_t>(p.min_spp) * P;
	AllocateArgs A{};
	A.error = error;
	A.mapOut = spp_map_out;
	A.W = c->cfg.width;
	A.localRows = c->localRows;
	A.rank = c->cfg.rank;
	A.nranks = c->cfg.nranks;
	A.localPixels = P;
	A.minSpp = p.min_spp;
	A.maxSpp = p.max_spp;
	A.extra = p.total > floorTotal ? static_cast<uint32_t>(p.total - floorTotal) : 0u;
	A.scan = c->dAllocScratch;
	A.blockSum = c->dAllocScratch + P;
	A.maxBits = reinterpret_cast<uint32_t*>(words);
	A.totalOut = words + 1;
	launch_allocate(A, s);
	if (int rc = L.close())
		return rc;
	if (total_out) {
		unsigned long long t = 0;
		HIPCHK(hipMemcpyAsync(&t, words + 1, sizeof t, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		*total_out = t;
	}
	return TYR_OK;
}

} // extern "C"
