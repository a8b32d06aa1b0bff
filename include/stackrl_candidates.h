/* stackrl_candidates.h — C-ABI of libstackrl_candidates.so: the candidates of a lookahead, spread over the value map by greedy
 * non-maximum suppression and picked on the device.
 *
 * `lookahead.candidates` takes the base policy's action and the k - 1 best other entries of its value map.  On a smooth map
 * those are the pixels next to the best one, so the physics is asked the same question k times.  Here a chosen entry strikes
 * the entries within a radius of it, and the next candidate is the best entry left.
 *
 * THE DEFINITION (stated here once; tests/candidates_cases.py restates it in numpy)
 *
 *   values is [B][G][A], float32 or float64, A = OH * OH, OH = H - h + 1 (the layout of stackrl_valueview.h and
 *   stackrl_compare.h).  The flat index of an entry is i = g * A + y * OH + x.  Only the maps g < n_valid are considered
 *   (1 <= n_valid <= G).  1 <= k <= SRL_CANDIDATES_MAX_K.  radius >= 0.  action is int64 [B] or NULL; it is device data, which the host cannot check without a synchronise, so the kernel clamps it to 0..G*A-1.  It may name a map
 *   >= n_valid.
 *
 *   1. Order of the considered entries.  Entry i ranks before entry j if v[i] is NaN and v[j] is not; otherwise, if neither is
 *      NaN, if v[i] > v[j]; otherwise (both NaN, or equal) if i < j.  The comparison is made in the type given (float64 is not
 *      narrowed: that would make ties that are not there).  -0 == +0.  -inf is an ordinary value, which ranks last.  This is
 *      the order of `torch.sort(descending=True, stable=True)`.
 *   2. Greedy choice.  Candidate 0 is action[b] (clamped); without action it is the first entry of the order.  Candidate c
 *      (c >= 1) is the first entry of the order that no candidate 0..c-1 suppresses.  A chosen entry (g, y, x) suppresses every
 *      entry (g, y', x') of the SAME map with max(|y - y'|, |x - x'|) <= radius, itself included.  Entries of different maps
 *      never suppress each other: another orientation or another rock is another placement.  (An action in a map >= n_valid
 *      therefore suppresses nothing that is considered.)
 *   3. Exhaustion.  If fewer than k entries can be chosen, count[b] is the number chosen (>= 1) and the slots
 *      count[b]..k-1 repeat candidate 0.  (`lookahead.choose` breaks ties to the lower rank, so a repeat never wins; it costs an
 *      evaluated slot, which count makes visible.)  A k beyond the n_valid * A entries considered is exhaustion by itself,
 *      and is served the same way (`lookahead.candidates` refuses it).
 *   4. Output.  cand is int64 [B][k], count is int32 [B].  Every element is written by the call, by plain stores: the same
 *      inputs give the same outputs.
 *   5. At radius 0, with k <= n_valid * A and an action in 0..G*A-1, the result is
 *      `lookahead.candidates(action, values, k, n_valid, A)` bit for bit, and count is k.  (That function passes an action outside 0..G*A-1 through as it is; the kernel clamps it, see
 *      above.  Where anything else here disagrees with that function at radius 0, the function is right.)  The function is
 *      `torch.sort`, and on a HIP device `torch.sort` ranks a NaN whose sign bit is set LAST, after -inf, where on the CPU it
 *      ranks every NaN first; point 1 is the CPU's order, so on device tensors the equality holds for maps whose NaNs have
 *      the sign bit clear (what the device's own arithmetic produces), and for every map against the function on CPU copies.
 *
 * One kernel, one path: one workgroup of SRL_CANDIDATES_THREADS threads per env, the values read where they lie (no scratch,
 * so there is no scratch-size export and no plan export).
 *
 * Plain C, device pointers owned by the caller, contiguous, `stream` is a hipStream_t as void*; returns 0 on success.
 */
#ifndef STACKRL_CANDIDATES_H_
#define STACKRL_CANDIDATES_H_

#include <stdint.h>

#include "srl_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRL_CANDIDATES_MAX_K 32
#define SRL_CANDIDATES_THREADS 1024

/* The candidates of B envs.  Enqueues one kernel on `stream`, allocates nothing, returns.  values is float64 where f64 is not
 * 0, else float32.  Returns 1 (SRL_EINVAL), with a text of its own behind srl_candidates_last_error and before any HIP call,
 * for: B, G or OH < 1; G * A beyond 2^31-2; n_valid outside 1..G; k outside 1..32; radius < 0; null values, cand or count.  A launch error returns 4 (SRL_EHIP). */
int srl_candidates_select(const void* values_dev,      /* [B][G][A] */
                          int32_t f64,
                          const int64_t* action_dev,   /* NULL, or [B] */
                          int32_t B, int32_t G, int32_t OH, int32_t n_valid, int32_t k, int32_t radius,
                          int64_t* cand_dev,           /* [B][k] */
                          int32_t* count_dev,          /* [B] */
                          void* stream);

const char* srl_candidates_last_error(void);
const char* srl_candidates_build_info(void);

#ifdef __cplusplus
}
#endif
#endif  /* STACKRL_CANDIDATES_H_ */
