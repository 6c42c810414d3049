/* ufm_score.h -- trajectory scoring, a part of the C ABI of libufm.so: included by ufm.h behind its last declaration (it needs ufm_t and
 * ufm_batch_t); including it alone includes ufm.h.  Plain C. */
#ifndef UFM_SCORE_H
#define UFM_SCORE_H
#include "ufm.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- trajectory scoring (no reference counterpart): what the CALLER's polylines cost on the raster the engine plans on, and whether
 * they are blocked -- candidate arcs of a local planner, the rollouts of a sampling controller, the path a supervisor is following --
 * without the raster leaving the device.  The charging rule is the extractor's: a move costs cell cost x length inside the cell.
 * A path is a polyline of n >= 0 points (x, y) in the frame of ufm_extract_paths_from: x the row in 0 .. length, y the column in
 * 0 .. width.  Its cost is the sum, over its segments in order, of the cost of each PIECE:
 *   pieces      a segment a -> b is cut at every crossing with a grid line x = k or y = j; the stretches between consecutive cuts are
 *               its pieces.  A stretch shorter than UFM_SCORE_MIN_PIECE cell sides is no piece: neither charged nor able to block (a
 *               segment through a vertex does not touch the two cells it meets in that point only).
 *   charge      a piece is charged length x cost of the cell that holds its midpoint, (floor(mx), floor(my)).  A segment that LIES on a
 *               grid line (ax == bx, an integer, or the same in y) runs between two cells: each of its pieces is charged the cheaper
 *               of the two that can be charged (the extractor with indirect traversals does the same).
 *   chargeable  a cell can be charged iff it is inside the raster and its byte is below the occupancy threshold (v >= thr cannot).
 *   the raster  the planning raster: what ufm_read_map returns -- dilated when a footprint is set, composed when there are layers.
 *   blocked     a piece that cannot be charged makes the path blocked; the first one in path order gives blocked_segment (the index of
 *               its segment), blocked_at (the segment's parameter t in [0, 1] where that piece begins) and cost_before (the cost of all
 *               pieces before it); cost is then +inf.  A free path has blocked_segment = -1, blocked_at = 0, cost_before = cost.
 *   end points  a segment with a non-finite end point, or one that starts outside [0, length] x [0, width], is blocked at t = 0 without
 *               being walked; one that leaves the map is blocked where it leaves.  No input makes a segment's walk longer than
 *               length + width + 2 pieces.
 *   dist        the length of the whole polyline, blocked or not; segments with a non-finite end point count as 0.
 *   pieces      the number of pieces charged (a blocked path: those before the blocked one).
 *   degenerate  zero-length segments, one-point paths and empty paths cost 0 and are free.
 * Arithmetic: cut parameters, piece lengths, the sum of a segment's pieces in walking order and the sum of the segments in index order
 * are fp64; cost, cost_before, dist and blocked_at are narrowed to fp32 once.  The order of summation depends on the path alone, so a
 * path's record is bit-identical whether it is scored alone or anywhere among others, on a planner, a batch or a sharded handle.
 * READ-ONLY: needs a map and nothing else -- no goal, no start, no step.  Patches that are being held (a single planner's small host
 * patches, a batch's "defer_patches") are applied first, as by ufm_extract_path; the field, the queues, the start, the statistics of
 * the next step, the step-delta baseline and the census are untouched.
 * ufm_score_paths: path k is points offsets[k] .. offsets[k + 1] - 1 of points_xy; out: [n_paths].  One wavefront per path, one launch
 * per 65 536 paths.  UFM_ERR_INVALID for the whole call, before anything is launched or written: a NULL handle or buffer, n_paths < 1,
 * offsets[0] != 0, decreasing offsets, no map.  Coordinates are never rejected: the rules above cover them.
 * ufm_score_paths_device: offsets, points and records in device memory on the map's device (rollouts a tensor library produced);
 * stream-ordered on ufm_stream: the call queues the work and returns, nothing is copied and nothing waited for.  total_points is the
 * number of points dev_points_xy holds: the kernel clamps every offset to [0, total_points] and reads a decreasing pair as an empty
 * path, so that no offsets can make it read outside the buffers.  UFM_ERR_INVALID: a NULL handle or buffer, n_paths < 1,
 * total_points < 0, no map. ---- */
typedef struct ufm_score {
    float cost;               /* +inf: blocked */
    float cost_before;        /* the cost of the pieces before the blocked one; a free path: cost */
    float dist;
    float blocked_at;
    int32_t blocked_segment;  /* -1: free */
    int32_t pieces;
} ufm_score;
#define UFM_SCORE_MIN_PIECE 9.5367431640625e-07   /* 2^-20 */
int ufm_score_paths(ufm_t *p, int n_paths, const int32_t *offsets /* [n_paths + 1] */, const float *points_xy /* [offsets[n_paths]][2] */,
                    ufm_score *out);
int ufm_score_paths_device(ufm_t *p, int n_paths, int total_points, const int32_t *dev_offsets, const float *dev_points_xy,
                           ufm_score *dev_out);
/* as ufm_score_paths: path k lies on map map_index[k] (int32 [n_paths], in any order, a map as often as the caller likes).
 * UFM_ERR_INVALID also for a NULL map_index, an index outside the batch or a named map without a raster -- before anything is written.
 * A sharded handle groups the paths by the device that owns their map and returns the records in the caller's order.
 * ufm_batch_score_paths_device scores all its paths on ONE map, i, whose device holds the three buffers; stream-ordered on that
 * shard's ufm_batch_stream. */
int ufm_batch_score_paths(ufm_batch_t *b, int n_paths, const int32_t *map_index, const int32_t *offsets, const float *points_xy,
                          ufm_score *out);
int ufm_batch_score_paths_device(ufm_batch_t *b, int i, int n_paths, int total_points, const int32_t *dev_offsets,
                                 const float *dev_points_xy, ufm_score *dev_out);

#ifdef __cplusplus
}
#endif
#endif /* UFM_SCORE_H */
