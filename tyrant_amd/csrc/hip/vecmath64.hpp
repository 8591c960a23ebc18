// vecmath64.hpp -- the binary64 triple of the units whose contracts are stated in binary64 (hip/segment.hip, sweep.hip,
// tri.hip, box.hip, winding.hip): device code only.  Every function is the operations it shows in the order it shows them,
// one IEEE binary64 operation each, because the tests' restatements (tests/*_ref.py) repeat them word for word:
//   dotd     (a.x * b.x + a.y * b.y) + a.z * b.z
//   crossd   (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x)
//   clamp01  v > 0 ? v : 0, then < 1 ? that : 1     (a NaN becomes 0)
//   mind     b < a ? b : a                          (of a NaN and a number: a)
//   maxd     b > a ? b : a
#pragma once

#include <hip/hip_runtime.h>

// one IEEE operation per source operation, also if a build forgets -ffp-contract=off
#pragma clang fp contract(off)

namespace tyr {

struct d3 {
	double x, y, z;
};

__device__ __forceinline__ d3 mk3d(double x, double y, double z) { return d3{ x, y, z }; }
__device__ __forceinline__ d3 operator+(d3 a, d3 b) { return mk3d(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ d3 operator-(d3 a, d3 b) { return mk3d(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ d3 operator*(double s, d3 a) { return mk3d(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ double dotd(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ d3 crossd(d3 a, d3 b) { return mk3d(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ double clamp01(double v) {
	const double v1 = v > 0 ? v : 0.0;
	return v1 < 1 ? v1 : 1.0;
}
__device__ __forceinline__ double mind(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double maxd(double a, double b) { return b > a ? b : a; }

} // namespace tyr
