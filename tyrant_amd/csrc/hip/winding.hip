// winding.hip -- generalised winding numbers of the ctx's scene (include/tyr_c.h "Winding numbers", DESIGN.md "Winding
// numbers"): the device build of the moment tree beside the scene, and k_winding, the stackless walk that sums a point's
// series.  Everything is binary64, one IEEE operation per operation of the contract (-ffp-contract=off), and every sum's
// order is the contract's, so a numpy restatement reproduces each word (tests/winding_ref.py).
#include "winding.hpp"

#include "detmath.hpp"
#include "vecmath64.hpp"
#include "winding_walk.hpp"

namespace tyr {
namespace {

constexpr int kB = 256;

// ---- the moment tree -------------------------------------------------------------------------------------------------------
// Pass 1: every interior node names itself to its two children.  Pass 2: one lane per leaf folds its triangles, then walks
// towards the root; at each parent the first arrival stops and the second adds the two children -- the contract fixes each
// node's operands, so which lane arrives second does not change a bit.  What one lane hands to another inside the launch (a
// node's seven moment words) is stored and loaded with agent-scope atomics, which go through to memory past the XCDs' private
// L2s, and is drained (vmcnt(0)) in front of the arrival count; the records themselves are read by later launches only.

struct Moments {
	d3 N;
	double S;
	d3 M;
};

__device__ __forceinline__ void put_moments(unsigned long long* m, const Moments& v) {
	const double w[7] = { v.N.x, v.N.y, v.N.z, v.S, v.M.x, v.M.y, v.M.z };
#pragma unroll
	for (int k = 0; k < 7; ++k)
		__hip_atomic_store(m + k, (unsigned long long)__double_as_longlong(w[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ Moments get_moments(const unsigned long long* m) {
	double w[7];
#pragma unroll
	for (int k = 0; k < 7; ++k)
		w[k] = __longlong_as_double((long long)__hip_atomic_load(m + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
	return Moments{ mk3d(w[0], w[1], w[2]), w[3], mk3d(w[4], w[5], w[6]) };
}

__global__ void __launch_bounds__(kB) k_winding_parents(WindingBuildArgs A) {
	const int i = blockIdx.x * kB + threadIdx.x;
	if (i >= A.nNodes)
		return;
	const tyr_bvh_node nd = A.src[i];
	if (nd.primitiveCount > 0 || nd.offset <= i + 1 || nd.offset >= A.nNodes) // (a leaf; or not a tree the layout pass accepts)
		return;
	A.parent[i + 1] = i;
	A.parent[nd.offset] = i;
}

// the index behind i's subtree: the offset of the first ancestor-or-self that is a left child's parent, else nNodes
__device__ __forceinline__ uint32_t skip_of(const WindingBuildArgs& A, int i) {
	for (int j = i; j > 0;) {
		const int pj = A.parent[j];
		if (pj < 0 || pj >= j)
			break;
		if (j == pj + 1)
			return (uint32_t)A.src[pj].offset;
		j = pj;
	}
	return (uint32_t)A.nNodes;
}

// node i's record from its moments and its box
__device__ __forceinline__ void write_node(const WindingBuildArgs& A, int i, const tyr_bvh_node& nd, const Moments& m) {
	const d3 lo = mk3d((double)nd.bbox.bounds[0][0], (double)nd.bbox.bounds[0][1], (double)nd.bbox.bounds[0][2]);
	const d3 hi = mk3d((double)nd.bbox.bounds[1][0], (double)nd.bbox.bounds[1][1], (double)nd.bbox.bounds[1][2]);
	const d3 p = m.S > 0.0 ? mk3d(m.M.x / m.S, m.M.y / m.S, m.M.z / m.S) : 0.5 * (lo + hi);
	const d3 dl = lo - p, dh = hi - p;
	const double r2 = (maxd(dl.x * dl.x, dh.x * dh.x) + maxd(dl.y * dl.y, dh.y * dh.y)) + maxd(dl.z * dl.z, dh.z * dh.z);
	WindingNode o;
	o.p[0] = p.x, o.p[1] = p.y, o.p[2] = p.z;
	o.N[0] = m.N.x, o.N[1] = m.N.y, o.N[2] = m.N.z;
	o.r2 = r2;
	const bool leaf = nd.primitiveCount > 0 && nd.offset >= 0 && (uint32_t)nd.offset + nd.primitiveCount <= A.nPrims;
	o.a = leaf ? (uint32_t)nd.offset : (nd.primitiveCount > 0 ? (uint32_t)i + 1u : skip_of(A, i));
	o.b = leaf ? (uint32_t)nd.primitiveCount : 0u;
	A.nodes[i] = o;
	A.S[i] = m.S;
}

__global__ void __launch_bounds__(kB) k_winding_moments(WindingBuildArgs A) {
	int i = blockIdx.x * kB + threadIdx.x;
	if (i >= A.nNodes)
		return;
	tyr_bvh_node nd = A.src[i];
	if (nd.primitiveCount == 0)
		return;
	Moments m{ mk3d(0.0, 0.0, 0.0), 0.0, mk3d(0.0, 0.0, 0.0) };
	if (nd.offset >= 0 && (uint32_t)nd.offset + nd.primitiveCount <= A.nPrims) {
		for (uint32_t t = (uint32_t)nd.offset; t < (uint32_t)nd.offset + nd.primitiveCount; ++t) {
			d3 v, e1, e2;
			load_tri(A.tris, t, v, e1, e2);
			const d3 n = 0.5 * crossd(e1, e2);
			const double a = __builtin_sqrt(dotd(n, n));
			const d3 es = e1 + e2;
			const d3 c = v + mk3d(es.x / 3.0, es.y / 3.0, es.z / 3.0);
			m.N = m.N + n;
			m.S = m.S + a;
			m.M = m.M + a * c;
		}
	}
	for (;;) {
		write_node(A, i, nd, m);
		put_moments(A.moments + 8 * (size_t)i, m);
		const int p = A.parent[i];
		if (p < 0 || p >= i)
			break;
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		if (__hip_atomic_fetch_add(&A.arrived[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
			break;
		asm volatile("" ::: "memory");
		nd = A.src[p];
		const Moments l = get_moments(A.moments + 8 * (size_t)(p + 1)), r = get_moments(A.moments + 8 * (size_t)nd.offset);
		m.N = l.N + r.N;
		m.S = l.S + r.S;
		m.M = l.M + r.M;
		i = p;
	}
}

// ---- the query -------------------------------------------------------------------------------------------------------------

// One point per lane, points in the batch's order (256 consecutive points per block); the walk is hip/winding_walk.hpp's, which
// hip/signed.hip shares.
__global__ void __launch_bounds__(kB) k_winding(WindingParams P) {
	const uint32_t g = blockIdx.x * (uint32_t)kB + threadIdx.x;
	if (g >= P.n)
		return;
	const float* pt = P.points + 3 * (size_t)g;
	const float fx = pt[0], fy = pt[1], fz = pt[2];
	uint32_t dipoles = 0, triangles = 0;
	float w = __uint_as_float(0x7fc00000u);
	if (finite32(fx) && finite32(fy) && finite32(fz)) {
		const d3 q = mk3d((double)fx, (double)fy, (double)fz);
		const double B2 = (double)P.accuracy * (double)P.accuracy;
		const uint32_t nNodes = (uint32_t)P.nNodes;
		const WindingSum s = winding_sum(P.nodes, P.tris, nNodes, q, B2);
		dipoles = s.dipoles, triangles = s.triangles;
		w = (float)(s.sum * dm::kInv4Pi);
	}
	P.w[g] = w;
	if (P.terms) {
		P.terms[2 * (size_t)g + 0] = dipoles;
		P.terms[2 * (size_t)g + 1] = triangles;
	}
}

inline unsigned blocks_for(size_t n) { return static_cast<unsigned>((n + kB - 1) / kB); }

} // namespace

void launch_winding_build(const WindingBuildArgs& A, hipStream_t stream) {
	if (A.nNodes <= 0)
		return;
	const unsigned blocks = blocks_for(static_cast<size_t>(A.nNodes));
	hipLaunchKernelGGL(k_winding_parents, dim3(blocks), dim3(kB), 0, stream, A);
	hipLaunchKernelGGL(k_winding_moments, dim3(blocks), dim3(kB), 0, stream, A);
}

void launch_winding(const WindingParams& P, hipStream_t stream) {
	if (P.n > 0)
		hipLaunchKernelGGL(k_winding, dim3(blocks_for(P.n)), dim3(kB), 0, stream, P);
}

} // namespace tyr
