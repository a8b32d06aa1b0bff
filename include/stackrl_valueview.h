/* stackrl_valueview.h — C-ABI of libstackrl_valueview.so: the frames of a visualised comparison run, drawn on the device.
 *
 * The reference's `run(..., visualize=True)` (`stackrl/test.py:230-317`) shows, at every step, the overhead view, the object
 * view and the value map of every policy (`ax.imshow(values[j, i].reshape(vshape))`: the default colour map, each map scaled
 * by itself), the driving policy's map framed in yellow (:252, :310-312).  Here one call draws that picture for n envs of a
 * batch as uint8 frames, from the images `env.render('rgb_array', dtype='uint8')` wrote and the policies' value maps where
 * they lie.
 *
 * THE DEFINITION (stated here once; tests/value_view_cases.py restates it in numpy)
 *
 *   One call draws n frames, frame f for env b = indexes[f] (clamped to 0..B-1: the indexes are device data, which the host
 *   cannot check without a synchronise; repeats are fine).  A = OH * OH actions, OH = H - h + 1.
 *
 *   1. Chosen row.  Policy j's maps are [B][G][A].  With actions (int64 [P][B]): row = actions[j][b] / A clamped to 0..G-1 and
 *      pixel = actions[j][b] mod A (the non-negative remainder).  Without: row 0, and nothing is marked.  What is coloured is
 *      the element rounded to float32, x (test.py:221-224, :277-280).
 *   2. Colour of a cell: matplotlib's `ScalarMappable.to_rgba(x, bytes=True)` with the default norm and `viridis`.
 *        vmin, vmax = the minimum and maximum over the FINITE cells of the map;
 *        in float32, one rounding per written operation:  t = x - vmin;  t = t / (vmax - vmin);  t = t * 256;
 *        t = 0 if vmax == vmin;   k = (int)t (truncation) clamped to 0..255, so x == vmax gives 255 (a NaN t gives 0);
 *        colour = LUT[k],  LUT[k][c] = (uint8)(viridis[k][c] * 255) (truncation), viridis = matplotlib's 256-entry table.
 *      A cell that is not finite, and every cell of a map without a finite cell, has the background colour.  If vmax - vmin
 *      overflows float32 the result is what IEEE arithmetic gives for the lines above.
 *   3. Window of policies shown (test.py:234-245, :294-295): nv = min(P, 6), min_j = clip(index - nv / 2, 0, P - nv); tile k
 *      (0..nv-1) shows policy min_j + k.  One line of tiles if nv <= 3, else two lines of 3: tile k sits in line k / 3,
 *      column k % 3.
 *   4. Layout, all integers, background (255, 255, 255).  g = 8 (SRL_VALUEVIEW_GAP), bw = 3 (SRL_VALUEVIEW_BORDER), s = scale:
 *        SH = s H, Sh = s h, ST = s OH, TB = ST + 2 bw, ncol = min(nv, 3), nline = 1 + (nv > 3),
 *        FW = 2 g + SH + ncol (TB + g),   FH = max(3 g + SH + Sh, g + nline (TB + g)).
 *      Overhead view: rows g .. g + SH, columns g .. g + SH, each source pixel an s x s block.  Object view: rows
 *      2 g + SH .. 2 g + SH + Sh, columns g .. g + Sh, likewise.  Tile k: its box of TB x TB starts at row
 *      g + (k / 3)(TB + g), column 2 g + SH + (k % 3)(TB + g); the map is the box minus a ring of width bw, each cell an
 *      s x s block.  The ring is (253, 231, 36) — the reference's (0.993248, 0.906157, 0.143936), LUT[255] — if the tile's
 *      policy is `index`, else background.  There is no text in a frame.
 *   5. Marks (mark = 1 and actions given; not in the reference).  In every tile the cell `pixel` of that tile's policy is
 *      (255, 0, 0).  In the overhead view the outline, one source pixel wide, of the h x h window of the DRIVING policy's
 *      pixel is (255, 0, 0): rows u .. u + h - 1, columns v .. v + h - 1, (u, v) = divmod(pixel, OH).
 *   6. Output: uint8 [n][FH][FW][3], contiguous.  Every byte is written by the call, by plain stores: the same inputs give
 *      the same bytes.
 *
 * Plain C, device pointers owned by the caller, contiguous, `stream` is a hipStream_t as void*; returns 0 on success.
 */
#ifndef STACKRL_VALUEVIEW_H_
#define STACKRL_VALUEVIEW_H_

#include <stdint.h>

#include "srl_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRL_VALUEVIEW_MAX_POLICIES 8   /* SRL_COMPARE_MAX_POLICIES */
#define SRL_VALUEVIEW_MAX_SHOWN 6      /* two lines of MAX_LINE_VISUALIZE = 3 (test.py:234) */
#define SRL_VALUEVIEW_MAX_SCALE 8
#define SRL_VALUEVIEW_GAP 8
#define SRL_VALUEVIEW_BORDER 3

/* The layout of a frame (host only, no device): out = FH, FW, nv, ncol, nline, TB, and the two ends of the window,
 * min_j for index = 0 (which is 0) and for index = P - 1 (which is P - nv).  The one place the layout arithmetic lives.
 * Returns 1 (SRL_EINVAL) for h < 1, H < h, P outside 1..8, scale outside 1..8, a null `out`, or a frame beyond 2^31-1 bytes. */
int srl_valueview_layout(int32_t H, int32_t h, int32_t P, int32_t scale, int32_t* out /* [8] */);

/* min_j of the window for driving policy `index` (host only).  Returns 1 for P outside 1..8, index outside 0..P-1 or null. */
int srl_valueview_window(int32_t P, int32_t index, int32_t* min_j);

/* The 256 x 3 bytes of the table the kernels use (host only). */
int srl_valueview_lut(uint8_t* out /* [768] */);

/* n frames.  Enqueues two kernels on `stream`, allocates nothing, returns.  map j is float64 where bit j of f64_mask is set,
 * else float32 (the convention of srl_compare_step); maps beyond P are not read.  Returns 1 (SRL_EINVAL), with a text of its
 * own behind srl_valueview_last_error and before any HIP call, for: P outside 1..8; index outside 0..P-1; scale outside 1..8;
 * n, B or G < 1; h < 1 or H < h; G * A beyond 2^31-2; a null pointer among the first P maps; null rgb0, rgb1, indexes,
 * range_scratch or frames; n * FH * FW * 3 beyond 2^31-1; frames_dev not 4-byte aligned (the frames are stored as 32-bit words).
 * A launch error returns 4 (SRL_EHIP). */
int srl_valueview_frames(int32_t P,
                         const void* map0, const void* map1, const void* map2, const void* map3,
                         const void* map4, const void* map5, const void* map6, const void* map7,   /* [B][G][A] each */
                         int32_t f64_mask, int32_t B, int32_t G, int32_t H, int32_t h,
                         const uint8_t* rgb0_dev,      /* [B][H][H][3] */
                         const uint8_t* rgb1_dev,      /* [B][h][h][3] */
                         const int64_t* actions_dev,   /* NULL, or [P][B]: row * A + pixel */
                         const int32_t* indexes_dev,   /* [n]: the env of each frame (clamped to 0..B-1 by the kernels) */
                         int32_t n, int32_t index, int32_t scale, int32_t mark,
                         float* range_scratch_dev,     /* [P][n][2]: (vmin, vmax) of the maps shown, (+inf, -inf) for no finite cell */
                         uint8_t* frames_dev,          /* [n][FH][FW][3] */
                         void* stream);

const char* srl_valueview_last_error(void);
const char* srl_valueview_build_info(void);

#ifdef __cplusplus
}
#endif
#endif  /* STACKRL_VALUEVIEW_H_ */
