// refit.hip -- tyr_scene_refit's kernels: new triangles in the uploaded tree's shape.  The boxes follow the reference's rule
// (a leaf: Union folded from BBox{} over its primitives' boxes in array order, bvh.cpp:71-73; an interior node: Union(left,
// right), bvh.cpp:222) with glibc's fmin / fmax (the first argument wins ties, as hip/bvh_build_dev.hip's), and land in the
// quad / pair records at the slots the upload's layout pass recorded (hip/refit.hpp RefitPlan).  Launch order:
//   k_refit_validate   one thread per triangle: non-finite geometry or boxes, a changed material / palette byte -> error bits;
//                      writes nothing else (the host reads the bits and stops before anything is changed)
//   k_refit_tris       the 48-byte triangle records
//   k_refit_subtrees   one block per subtree of the cut (at most kRefitRangeNodes nodes, a contiguous index range): leaf boxes
//                      from the primitives, then the interior nodes height by height in LDS -- a node's children lie inside
//                      its range, so nothing crosses blocks
//   k_refit_top        one block: the nodes above the cut, height by height (their children are range roots, written by the
//                      launch before, or top nodes of a lower height, written by this block)
//   k_refit_scatter    one thread per quad slot and per pair side: the box of its node into the record
// Every hand-off between blocks is a kernel boundary; the top's hand-offs inside its one block are L1-bypassing (sc1) stores and
// loads behind a vmcnt wait and a barrier.
#include <hip/hip_runtime.h>

#include "refit.hpp"

namespace tyr {

namespace {

constexpr int kB = 256;
constexpr int kPer = static_cast<int>(kRefitRangeNodes) / kB; // range nodes per thread
constexpr int kTopB = 1024;

__device__ __forceinline__ float fmin_first(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float fmax_first(float a, float b) { return (b > a) ? b : a; }
__device__ __forceinline__ bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the box of triangle i: the caller's, or Scene.cpp:22-33's (BBox{} grown by vert, vert + e1, vert + e2; host/bvh_build.cpp)
__device__ __forceinline__ void prim_box(const RefitArgs& A, int i, float* lo, float* hi) {
	if (A.bboxes) {
		const tyr_bbox b = A.bboxes[i];
		for (int k = 0; k < 3; ++k) {
			lo[k] = b.bounds[0][k];
			hi[k] = b.bounds[1][k];
		}
		return;
	}
	const tyr_triangle t = A.prims[i];
	for (int k = 0; k < 3; ++k) {
		const float v0 = t.vert[k], v1 = t.vert[k] + t.e1[k], v2 = t.vert[k] + t.e2[k];
		lo[k] = fmin_first(fmin_first(fmin_first(1e10f, v0), v1), v2);
		hi[k] = fmax_first(fmax_first(fmax_first(-1e10f, v0), v1), v2);
	}
}

__global__ void __launch_bounds__(kB) k_refit_validate(RefitArgs A) {
	const int i = blockIdx.x * kB + threadIdx.x;
	if (i >= A.n)
		return;
	const tyr_triangle t = A.prims[i];
	float lo[3], hi[3];
	prim_box(A, i, lo, hi);
	uint32_t bits = 0;
	if (!finite3(t.vert) || !finite3(t.e1) || !finite3(t.e2) || !finite3(lo) || !finite3(hi))
		bits |= kRefitErrNonFinite;
	const float4 w = A.tris[3 * (size_t)i + 2]; // .y = materialType, .z = the palette byte (offsets 36, 37)
	if (__float_as_uint(w.y) != (uint32_t)t.materialType || __float_as_uint(w.z) != (uint32_t)t.pad_[0])
		bits |= kRefitErrMaterial;
	if (bits)
		atomicOr(A.err, bits);
}

// bvh_layout.cpp "triangles": 40-byte records -> 3 x dwordx4
__global__ void __launch_bounds__(kB) k_refit_tris(RefitArgs A) {
	const int i = blockIdx.x * kB + threadIdx.x;
	if (i >= A.n)
		return;
	const tyr_triangle t = A.prims[i];
	float4* q = A.tris + 3 * (size_t)i;
	q[0] = make_float4(t.vert[0], t.vert[1], t.vert[2], t.e1[0]);
	q[1] = make_float4(t.e1[1], t.e1[2], t.e2[0], t.e2[1]);
	q[2] = make_float4(t.e2[2], __uint_as_float((uint32_t)t.materialType), __uint_as_float((uint32_t)t.pad_[0]), 0.0f);
}

__device__ __forceinline__ void store_box(tyr_bvh_node* node, const float* lo, const float* hi) {
	float* o = reinterpret_cast<float*>(node); // bbox at offset 0 of a 32-byte record
	*reinterpret_cast<float4*>(o) = make_float4(lo[0], lo[1], lo[2], hi[0]);
	*reinterpret_cast<float2*>(o + 4) = make_float2(hi[1], hi[2]);
}

__global__ void __launch_bounds__(kB) k_refit_subtrees(RefitArgs A) {
	__shared__ float slo[3][kRefitRangeNodes], shi[3][kRefitRangeNodes];
	const uint4 r = A.ranges[blockIdx.x];
	const int b = (int)r.x, n = (int)(r.y - r.x), hmax = (int)r.z;
	int h[kPer], kl[kPer], kr[kPer];
#pragma unroll
	for (int j = 0; j < kPer; ++j) {
		const int i = (int)threadIdx.x + j * kB;
		h[j] = -1;
		kl[j] = kr[j] = 0;
		if (i >= n)
			continue;
		const tyr_bvh_node nd = A.nodes[b + i];
		if (nd.primitiveCount > 0) {
			float lo[3] = { 1e10f, 1e10f, 1e10f }, hi[3] = { -1e10f, -1e10f, -1e10f }; // Bbox.h:5
			for (int p = nd.offset; p < nd.offset + (int)nd.primitiveCount; ++p) {
				float plo[3], phi[3];
				prim_box(A, p, plo, phi);
				for (int k = 0; k < 3; ++k) {
					lo[k] = fmin_first(lo[k], plo[k]);
					hi[k] = fmax_first(hi[k], phi[k]);
				}
			}
			for (int k = 0; k < 3; ++k) {
				slo[k][i] = lo[k];
				shi[k][i] = hi[k];
			}
			h[j] = 0;
		} else {
			h[j] = A.height[b + i];
			kl[j] = i + 1;
			kr[j] = nd.offset - b;
		}
	}
	__syncthreads();
	for (int lvl = 1; lvl <= hmax; ++lvl) {
#pragma unroll
		for (int j = 0; j < kPer; ++j) {
			if (h[j] != lvl)
				continue;
			const int i = (int)threadIdx.x + j * kB;
			for (int k = 0; k < 3; ++k) {
				slo[k][i] = fmin_first(slo[k][kl[j]], slo[k][kr[j]]);
				shi[k][i] = fmax_first(shi[k][kl[j]], shi[k][kr[j]]);
			}
		}
		__syncthreads();
	}
#pragma unroll
	for (int j = 0; j < kPer; ++j) {
		const int i = (int)threadIdx.x + j * kB;
		if (i >= n)
			continue;
		const float lo[3] = { slo[0][i], slo[1][i], slo[2][i] }, hi[3] = { shi[0][i], shi[1][i], shi[2][i] };
		store_box(&A.nodes[b + i], lo, hi);
	}
}

__device__ __forceinline__ float load_sc1(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_sc1(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(kTopB) k_refit_top(RefitArgs A) {
	for (uint32_t l = 0; l < A.nTopLevels; ++l) {
		const uint32_t end = A.topLevel[l + 1];
		for (uint32_t k = A.topLevel[l] + threadIdx.x; k < end; k += kTopB) {
			const int i = A.top[k];
			const float* L = reinterpret_cast<const float*>(&A.nodes[i + 1]);
			const float* R = reinterpret_cast<const float*>(&A.nodes[A.nodes[i].offset]);
			float* o = reinterpret_cast<float*>(&A.nodes[i]);
			for (int k2 = 0; k2 < 3; ++k2) {
				store_sc1(o + k2, fmin_first(load_sc1(L + k2), load_sc1(R + k2)));
				store_sc1(o + 3 + k2, fmax_first(load_sc1(L + 3 + k2), load_sc1(R + 3 + k2)));
			}
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
	}
}

__global__ void __launch_bounds__(kB) k_refit_scatter(RefitArgs A) {
	const uint32_t t = blockIdx.x * kB + threadIdx.x;
	int32_t node;
	float* q;
	uint32_t stride; // floats between the axes' pairs of planes
	if (t < A.nSlots) {
		node = A.slotNode[t];
		// q0 = {s0.min.x, s0.max.x, s1.min.x, s1.max.x}  q1 = {s2.., s3..}  q2,q3 = y  q4,q5 = z (bvh_layout.cpp quad_write)
		q = reinterpret_cast<float*>(A.quads) + (size_t)(t >> 2) * 32 + 2 * (t & 3u);
		stride = 8;
	} else if (t - A.nSlots < A.nPairSides) {
		const uint32_t s = t - A.nSlots;
		node = A.pairNode[s];
		// {l.min.x, l.max.x, r.min.x, r.max.x} per axis (bvh_layout.cpp pair_write)
		q = reinterpret_cast<float*>(A.pairs) + (size_t)(s >> 1) * 16 + 2 * (s & 1u);
		stride = 4;
	} else {
		return;
	}
	if (node < 0)
		return;
	const float* bx = reinterpret_cast<const float*>(&A.nodes[node]);
	for (int k = 0; k < 3; ++k)
		*reinterpret_cast<float2*>(q + stride * k) = make_float2(bx[k], bx[3 + k]);
}

inline unsigned blocks_for(size_t n) { return static_cast<unsigned>((n + kB - 1) / kB); }

} // namespace

void launch_refit_validate(const RefitArgs& A, hipStream_t stream) {
	if (A.n > 0)
		hipLaunchKernelGGL(k_refit_validate, dim3(blocks_for(static_cast<size_t>(A.n))), dim3(kB), 0, stream, A);
}

void launch_refit(const RefitArgs& A, uint32_t nRanges, hipStream_t stream) {
	if (A.n > 0)
		hipLaunchKernelGGL(k_refit_tris, dim3(blocks_for(static_cast<size_t>(A.n))), dim3(kB), 0, stream, A);
	if (nRanges > 0)
		hipLaunchKernelGGL(k_refit_subtrees, dim3(nRanges), dim3(kB), 0, stream, A);
	if (A.nTopLevels > 0)
		hipLaunchKernelGGL(k_refit_top, dim3(1), dim3(kTopB), 0, stream, A);
	const size_t nScatter = static_cast<size_t>(A.nSlots) + A.nPairSides;
	if (nScatter > 0)
		hipLaunchKernelGGL(k_refit_scatter, dim3(blocks_for(nScatter)), dim3(kB), 0, stream, A);
}

} // namespace tyr
