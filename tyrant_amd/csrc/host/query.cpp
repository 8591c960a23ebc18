// query.cpp -- tyr_query_closest / tyr_query_any / tyr_query_error: batched ray queries on the ctx's scene (include/tyr_c.h
// "ray queries"; the kernels are hip/query.hip).  Nothing here reads or writes render state: the queries have device words of
// their own (the error bits and the chunk tickets) and run on the caller's stream.
//
// Tickets.  A launch hands out its rays through one ticket word that must be zero when it starts.  Launches on one stream
// run one after another, so each stream the queries use gets a word of its own, cleared in front of every launch on that
// stream.  Once every word has an owner, the least recently used one changes hands, and its new stream first waits for
// the last launch that used it.
#include <hip/hip_runtime.h>

#include "../hip/query.hpp"
#include "driver_internal.hpp"

using namespace tyr;
using namespace tyr::drv;

namespace {

constexpr uint32_t kQueryWordStride = 32; // uint32 words between two device words (128 bytes: an L2 line each)
constexpr uint32_t kQueryTickets = 64;    // ticket words: streams served without a hand-over
// c->dQuery: the error bits at word 0, ticket word k at (k + 1) * kQueryWordStride
constexpr size_t kQueryWords = static_cast<size_t>(kQueryTickets + 1) * kQueryWordStride;

int query_words(tyr_ctx* c) {
	if (c->dQuery)
		return TYR_OK;
	if (int rc = dev_alloc(c->dQuery, kQueryWords))
		return rc;
	HIPCHK(hipMemset(c->dQuery, 0, kQueryWords * sizeof(uint32_t)));
	return TYR_OK;
}

// the entry of `stream` in c->queryStreams
int query_stream(tyr_ctx* c, hipStream_t stream, tyr_ctx::QueryStream*& out) {
	auto& v = c->queryStreams;
	for (auto& q : v) {
		if (q.stream == stream) {
			out = &q;
			return TYR_OK;
		}
	}
	if (v.size() < kQueryTickets) {
		hipEvent_t e = nullptr;
		HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		v.push_back({ stream, e, static_cast<uint32_t>(v.size()), 0 });
		out = &v.back();
		return TYR_OK;
	}
	auto* lru = &v[0];
	for (auto& q : v)
		if (q.lastUse < lru->lastUse)
			lru = &q;
	HIPCHK(hipStreamWaitEvent(stream, lru->done, 0));
	lru->stream = stream;
	out = lru;
	return TYR_OK;
}

int query_launch(tyr_ctx* c, bool any, uint32_t n, const float* origins, const float* directions, const float* tmax, uint32_t flags, float* t_out, int32_t* prim_out,
                 int32_t* geom_out, float* uv_out, uint8_t* occluded_out, void* stream) {
	if (!c || n >= (1u << 31) || (flags & ~TYR_QUERY_SPHERES) != 0u)
		return TYR_ERR_INVALID;
	if (!c->haveScene)
		return TYR_ERR_NO_SCENE;
	if (n == 0)
		return TYR_OK;
	if (!origins || !directions || (any ? !occluded_out : (!t_out || !prim_out)))
		return TYR_ERR_INVALID;
	QueryLaunch L;
	if (int rc = L.open(c, stream))
		return rc;

	QueryParams P{};
	query_fields(P, c, L);
	P.origins = origins;
	P.directions = directions;
	P.tmax = tmax;
	P.t = t_out;
	P.prim = prim_out;
	P.geom = geom_out;
	P.uv = uv_out;
	P.occluded = occluded_out;
	P.n = n;
	launch_query(P, any, (flags & TYR_QUERY_SPHERES) != 0u, c->numCUs, c->launchCache, L.s);
	return L.close();
}

} // namespace

namespace tyr {
namespace drv {

int QueryLaunch::open(tyr_ctx* c, void* stream) {
	if (scope.prev < 0) // (an entry's first launch)
		if (int rc = scope.enter(c))
			return rc;
	if (int rc = query_words(c))
		return rc;
	s = stream ? static_cast<hipStream_t>(stream) : c->stream;
	tyr_ctx::QueryStream* qs = nullptr;
	if (int rc = query_stream(c, s, qs))
		return rc;
	qs->lastUse = ++c->querySeq;
	done = qs->done;
	ticket = c->dQuery + (1 + qs->word) * kQueryWordStride;
	HIPCHK(hipMemsetAsync(ticket, 0, sizeof(uint32_t), s));
	return TYR_OK;
}

int QueryLaunch::close() {
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(done, s));
	return TYR_OK;
}

int query_wait(tyr_ctx* c) {
	for (const auto& q : c->queryStreams)
		HIPCHK(hipEventSynchronize(q.done));
	return TYR_OK;
}

void query_free(tyr_ctx* c) {
	(void)query_wait(c);
	for (auto& q : c->queryStreams)
		(void)hipEventDestroy(q.done);
	c->queryStreams.clear();
	dev_free(c->dQuery);
}

} // namespace drv
} // namespace tyr

int tyr_query_closest(tyr_ctx* ctx, uint32_t n, const float* origins, const float* directions, const float* tmax, uint32_t flags, float* t_out, int32_t* prim_out, int32_t* geom_out,
                      float* uv_out, void* stream) {
	return query_launch(ctx, false, n, origins, directions, tmax, flags, t_out, prim_out, geom_out, uv_out, nullptr, stream);
}

int tyr_query_any(tyr_ctx* ctx, uint32_t n, const float* origins, const float* directions, const float* tmax, uint32_t flags, uint8_t* occluded_out, void* stream) {
	return query_launch(ctx, true, n, origins, directions, tmax, flags, nullptr, nullptr, nullptr, nullptr, occluded_out, stream);
}

int tyr_query_error(tyr_ctx* ctx, uint32_t* bits_out, int reset) {
	if (!ctx || !bits_out)
		return TYR_ERR_INVALID;
	*bits_out = 0;
	if (!ctx->dQuery)
		return TYR_OK;
	DeviceScope scope;
	if (int rc = scope.enter(ctx))
		return rc;
	if (int rc = query_wait(ctx))
		return rc;
	HIPCHK(hipMemcpy(bits_out, ctx->dQuery, sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (reset)
		HIPCHK(hipMemset(ctx->dQuery, 0, sizeof(uint32_t)));
	return TYR_OK;
}
