/* ufm_cspace_graded.h -- the graded footprint of the C-space inflation, a part of the C ABI of libufm.so: included by ufm.h behind its
 * last declaration (it needs ufm_t and ufm_batch_t); including it alone includes ufm.h.  Plain C. */
#ifndef UFM_CSPACE_GRADED_H
#define UFM_CSPACE_GRADED_H
#include "ufm.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- graded footprint (no reference counterpart; the inflation layer of ROS costmap_2d / nav2 is the model): the footprint of
 * ufm_set_cspace is flat -- a cell inside the vehicle's disc takes the obstacle's full cost, a cell outside takes none, and paths run
 * exactly one radius from every wall.  A graded footprint adds a margin that decays with distance, kept exact under patches, reveals
 * and layers as the flat one is.  The reference's simulator blurs its bitmap once, before the mission; nothing found later gets a margin.
 * The footprint is drop[mh][mw], row-major uint8, with an anchor (anchor_row, anchor_col); -1, -1: the centre (mh / 2, mw / 2).
 * drop == UFM_CSPACE_OUTSIDE (255): the cell is no part of the footprint.  With a graded footprint set
 *     planning[i][j] = max { max(raw[i + a - anchor_row][j + b - anchor_col] - drop[a][b], 0)
 *                            : drop[a][b] != 255, the raw index inside the map }
 * -- grey-scale dilation by a non-flat structuring element, in integers: every raster stays exact.  Cells outside the map are ignored,
 * as by ufm_set_cspace.  Everything downstream is unchanged and reads this raster: the threshold, the operators, ufm_read_map, the
 * census, step deltas, ufm_score_paths, the path extractor.  ufm_set_map*, ufm_patch_map*, ufm_reveal, ufm_set_image* and the layer
 * calls take RAW data exactly as with a flat footprint, ufm_read_raw_map returns it, and the grown rectangle of a raw patch is the one
 * of the footprint's mh x mw box (ufm.h).
 * A valid footprint: drop non-NULL; 1 <= mw, mh <= 31; the anchor inside the matrix; drop[anchor] == 0, so that planning >= raw; at
 * most UFM_CSPACE_MAX_LEVELS distinct values other than 255.  Nothing else is asked of the drops: they need not be monotone.  Checked
 * before anything is launched, allocated or written: UFM_ERR_INVALID leaves the handle as it was and usable.
 * A property of the vehicle like the flat footprint: set after ufm_create and before the first ufm_set_map* / ufm_set_image*,
 * UFM_ERR_INVALID otherwise.  The last footprint call of either kind before the first raster wins: ufm_set_cspace replaces a graded
 * footprint, and the reverse.  Drops that all lie in {0, 255} leave the handle exactly as ufm_set_cspace(mask = drop != 255) would --
 * 1 x 1 is off, and off costs nothing.
 * ufm_batch_set_cspace_graded: one footprint for every map on every shard. ---- */
#define UFM_CSPACE_OUTSIDE 255
#define UFM_CSPACE_MAX_LEVELS 16
int ufm_set_cspace_graded(ufm_t *p, const uint8_t *drop, int mw, int mh, int anchor_row, int anchor_col);
int ufm_batch_set_cspace_graded(ufm_batch_t *b, const uint8_t *drop, int mw, int mh, int anchor_row, int anchor_col);
/* The cone footprint: host arithmetic only, no device, integers throughout.  r_in = inner_d / 2, r_out = outer_d / 2; drop is
 * [n][n], n = 2 * r_out + 1, anchor at its centre.  At offset (dx, dy) from the centre, d2 = dx * dx + dy * dy:
 *     d2 <= r_in * r_in:    0                   (the flat disc of diameter inner_d)
 *     d2 <= r_out * r_out:  min(254, step * k), k the smallest integer >= 1 with d2 <= (r_in + k) * (r_in + k)
 *     beyond:               255
 * UFM_ERR_INVALID for a NULL drop, inner_d < 1, inner_d > outer_d, r_out > 15, r_out - r_in > 15, or step outside 1 .. 254. */
int ufm_cspace_cone(int inner_d, int outer_d, int step, uint8_t *drop /* [n][n], n = 2 * (outer_d / 2) + 1 */);

#ifdef __cplusplus
}
#endif
#endif /* UFM_CSPACE_GRADED_H */
