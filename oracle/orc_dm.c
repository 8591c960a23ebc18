/*
 * oracle/orc_dm.c -- the deterministic transcendental layer (orc_internal.h dm_*) over arrays, with the binary64 values
 * each function rounds: what the device's probe ops 32-43 (hip/frame.hip contract_probe) are compared with, bit for bit
 * (tests/test_numeric_contract.py; DESIGN.md "Numeric contract").  TEST INFRASTRUCTURE (see orc.h).
 *
 * This file needs nothing but orc_internal.h, so that a test can compile it a second time with other floating-point
 * flags and see what a contracted build would change (tests/test_oracle_math.py).
 *
 * Each case restates the function's own lines with the function's own building blocks.  A value the function does not
 * reach for this argument (an early return) is 0.
 *
 *   op            out32[2*i ..]        out64[4*i ..]
 *   0 sin         result, q            r, the value that is rounded
 *   1 cos         result, q            r, the value that is rounded
 *   2 sin & cos   dm_sinf, dm_cosf     -
 *   3 exp         result, 0            kd, r, exp_poly(r) * pow2i(kd)
 *   4 pow(x, y)   result, 0            log2(x), t, w, exp_poly(w) * pow2i(kd)
 */
#include "orc_internal.h"

static inline uint32_t f32_bits(float f) {
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

int orc_dm_map(int op, const float* x, const float* y, int n, uint32_t* out32, double* out64) {
	if (op < 0 || op > 4 || (op == 4 && !y))
		return -1;
	for (int i = 0; i < n; ++i) {
		const float xf = x[i];
		uint32_t* o32 = out32 + 2 * (size_t)i;
		double* o64 = out64 + 4 * (size_t)i;
		o32[0] = o32[1] = 0u;
		o64[0] = o64[1] = o64[2] = o64[3] = 0.0;
		switch (op) {
		case 0:
		case 1: {
			o32[0] = f32_bits(op == 0 ? dm_sinf(xf) : dm_cosf(xf));
			if (!(fabsf(xf) < 1048576.0f))
				break;
			int q;
			double r = dm_reduce_pio2((double)xf, &q);
			o32[1] = (uint32_t)q;
			o64[0] = r;
			if (op == 0) {
				double s = (q & 1) ? dm_cos_poly(r) : dm_sin_poly(r);
				o64[1] = (q & 2) ? -s : s;
			} else {
				double c = (q & 1) ? dm_sin_poly(r) : dm_cos_poly(r);
				o64[1] = ((q + 1) & 2) ? -c : c;
			}
			break;
		}
		case 2:
			o32[0] = f32_bits(dm_sinf(xf));
			o32[1] = f32_bits(dm_cosf(xf));
			break;
		case 3: {
			o32[0] = f32_bits(dm_expf(xf));
			double xd = (double)xf;
			if (xf != xf || xd > 89.0 || xd < -104.0)
				break;
			double kd = dm_round(xd * 0x1.71547652b82fep+0);
			double r = (xd - kd * 0x1.62e42fee00000p-1) - kd * 0x1.a39ef35793c76p-33;
			o64[0] = kd;
			o64[1] = r;
			o64[2] = dm_exp_poly(r) * dm_pow2i((int)kd);
			break;
		}
		default: {
			const float yf = y[i];
			o32[0] = f32_bits(dm_powf(xf, yf));
			if (yf != yf || !(xf > 0.0f) || xf == INFINITY)
				break;
			double l2 = dm_log2((double)xf);
			double t = (double)yf * l2;
			o64[0] = l2;
			o64[1] = t;
			if (t > 129.0 || t < -152.0)
				break;
			double kd = dm_round(t);
			double w = (t - kd) * 0x1.62e42fefa39efp-1;
			o64[2] = w;
			o64[3] = dm_exp_poly(w) * dm_pow2i((int)kd);
			break;
		}
		}
	}
	return 0;
}
