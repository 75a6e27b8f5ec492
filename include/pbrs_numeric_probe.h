/* pbrs_numeric_probe.h — TEST INFRASTRUCTURE: the probes of include/pbrs_numeric.h that the device (k_numeric_eval,
 * k_numeric_eval_k) and the CPU oracle (oracle_numeric_eval, oracle_numeric_eval_k) share, so that both sides number and
 * unpack them alike.  Every result is a raw 32-bit word: the bits of an f32, or an integer where the function returns one.
 *
 * pn_probe_eval: fn ids from 16 on, one or two f32 operands (ids 0-15 live in the two callers).
 *   16 trunc   17 f32_to_i32 (word)   18 ldexp(a, (int)b)   19 max   20 min   21 signum   22 weak_recip
 *   23-26 pn_sincos_f64 of the f64 angle (double)a + (double)b: sin high word, sin low word, cos high word, cos low word
 *   27 rng_u32 (word) and 28 rng_f32 of the state whose low / high words are the BITS of a / b
 * pn_probe_eval_k: functions of up to PN_PROBE_MAX_K operands; `w` is one row of the operand matrix, as words.
 *   0 mul_add(a, b, c)   1 clamp(x, lo, hi)   2 slab_filter (its 13 operands in declaration order; word 0 / 1)
 *   3 / 4 low / high word of rng_init(seed = w[0] | w[1] << 32, pixel = w[2], sample = w[3]) (operands are integers)
 *   5 rng_u32 and 6 rng_f32: draw number w[4] & 1023 (from 0) of that stream
 */
#ifndef PBRS_NUMERIC_PROBE_H
#define PBRS_NUMERIC_PROBE_H

#include "pbrs_numeric.h"

#define PN_PROBE_FIRST 16u
#define PN_PROBE_LAST 28u
#define PN_PROBE_MAX_K 16u
#define PN_PROBE_K_LAST 6u

PN_FN uint32_t pn_probe_f64_word_(double d, int high) {
    uint64_t u;
    __builtin_memcpy(&u, &d, 8);
    return high ? (uint32_t)(u >> 32) : (uint32_t)u;
}

PN_FN uint32_t pn_probe_eval(uint32_t fn, float a, float b) {
    switch (fn) {
        case 16: return pn_bits(pn_trunc(a));
        case 17: return (uint32_t)pn_f32_to_i32(a);
        case 18: return pn_bits(pn_ldexp(a, (int)b));
        case 19: return pn_bits(pn_max(a, b));
        case 20: return pn_bits(pn_min(a, b));
        case 21: return pn_bits(pn_signum(a));
        case 22: return pn_bits(pn_weak_recip(a));
        case 23:
        case 24:
        case 25:
        case 26: {
            double s, c;
            pn_sincos_f64((double)a + (double)b, &s, &c);
            return pn_probe_f64_word_(fn < 25u ? s : c, (int)(fn & 1u));
        }
        case 27:
        case 28: {
            uint64_t st = ((uint64_t)pn_bits(b) << 32) | (uint64_t)pn_bits(a);
            return fn == 27u ? pn_rng_u32(&st) : pn_bits(pn_rng_f32(&st));
        }
        default: return 0u;
    }
}

PN_FN uint32_t pn_probe_eval_k(uint32_t fn, const uint32_t* w) {
    switch (fn) {
        case 0: return pn_bits(pn_mul_add(pn_from_bits(w[0]), pn_from_bits(w[1]), pn_from_bits(w[2])));
        case 1: return pn_bits(pn_clamp(pn_from_bits(w[0]), pn_from_bits(w[1]), pn_from_bits(w[2])));
        case 2:
            return (uint32_t)pn_slab_filter(pn_from_bits(w[0]), pn_from_bits(w[1]), pn_from_bits(w[2]), pn_from_bits(w[3]), pn_from_bits(w[4]),
                                            pn_from_bits(w[5]), pn_from_bits(w[6]), pn_from_bits(w[7]), pn_from_bits(w[8]), pn_from_bits(w[9]),
                                            pn_from_bits(w[10]), pn_from_bits(w[11]), pn_from_bits(w[12]));
        case 3:
        case 4:
        case 5:
        case 6: {
            uint64_t st = pn_rng_init(((uint64_t)w[1] << 32) | (uint64_t)w[0], w[2], w[3]);
            if (fn == 3u) return (uint32_t)st;
            if (fn == 4u) return (uint32_t)(st >> 32);
            for (uint32_t d = 0; d < (w[4] & 1023u); ++d) (void)pn_rng_u32(&st);
            return fn == 5u ? pn_rng_u32(&st) : pn_bits(pn_rng_f32(&st));
        }
        default: return 0u;
    }
}
/* operands each matrix function reads (0: no such function) */
PN_FN uint32_t pn_probe_k_operands(uint32_t fn) {
    return fn <= 1u ? 3u : fn == 2u ? 13u : fn <= 4u ? 4u : fn <= 6u ? 5u : 0u;
}

#endif /* PBRS_NUMERIC_PROBE_H */
