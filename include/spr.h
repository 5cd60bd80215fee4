/*
 * spr.h -- C ABI of libspr_hip.so, the MI355X (gfx950) implementation of the
 * Superpoints_Registration hot path.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - varlen batches are packed [sum N, C] row-major with cu_seqlens
 *     int32[n_seg + 1] (cu[0] = 0) on the device; clouds are stacked
 *     [src_0..src_{B-1}, tgt_0..tgt_{B-1}] as in qk_regtr_full.py:152;
 *   - `stream` is a hipStream_t passed as void*; all work is stream ordered,
 *     nothing synchronises, nothing allocates: scratch comes from the caller
 *     (`ws`, size from the matching *_workspace_bytes query: the query measures the very layout the
 *     entry point carves, so a buffer of that size is always accepted and a smaller one is refused,
 *     status 2, before anything is enqueued -- except where a note below names a smaller layout an entry
 *     point falls back to or needs: spr_attn_varlen_bwd, spr_bce_logits_mean, spr_transform_l1_pair);
 *   - return value 0 = success, anything else = failure; spr_last_error()
 *     returns a thread-local message.  The Python binding raises RuntimeError,
 *     which is what the reference's CPython modules raise
 *     (cpp_neighbors/wrapper.cpp:201-205, cpp_subsampling/wrapper.cpp:266-270).
 *
 * Each function cites the reference interface it replaces (paths relative to
 * /root/reference/src).
 */
#ifndef SPR_H_
#define SPR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPR_VERSION 6

/* activation codes for spr_linear / spr_instnorm */
#define SPR_ACT_NONE 0
#define SPR_ACT_RELU 1
#define SPR_ACT_SIGMOID 2

/* output ordering of spr_grid_subsample */
#define SPR_ORDER_REFERENCE 0 /* libstdc++ unordered_map iteration order     */
#define SPR_ORDER_CANONICAL 1 /* ascending (cloud, voxel key)                 */

/* a2 selection rule: which `limit` of a query's supports in range a row keeps */
#define SPR_SELECT_NEAREST 0 /* smallest (d2, index), ascending: cpp_neighbors */
#define SPR_SELECT_INDEX 1   /* smallest indices, ascending: pytorch3d ball_query */

int spr_version(void);
const char* spr_last_error(void);

/* ---- a1: grid subsampling ------------------------------------------------
 * Replaces grid_subsampling.subsample_batch(points, batches, sampleDl=, max_p=)
 * (models/backbone_kpconv/cpp_wrappers/cpp_subsampling/wrapper.cpp:62-82 ->
 *  grid_subsampling/grid_subsampling.cpp:109 batch_grid_subsampling), called
 * from models/backbone_kpconv/kpconv.py:174-185 (and the GPU variant :217).
 * Barycentres are bit-exact float32 (in-order sum * (float)(1.0/count)).
 * Voxel keys are the reference's size_t keys, also for a point below the grid
 * origin (the float32 origin can round to one ulp above the cloud's minimum):
 * cell index -1, key arithmetic modulo 2^64.  SPR_ORDER_CANONICAL orders by
 * that 64-bit key.  *out_total = -1: the grid needs keys beyond 2^40.
 *   xyz      [n,3] f32        cu [nb+1] i32
 *   out_xyz  [n,3] f32 (first *out_total rows valid)
 *   out_lens [nb] i32         out_total [1] i32 (both device)
 */
size_t spr_grid_subsample_workspace_bytes(int n, int nb);
int spr_grid_subsample(const float* xyz, const int* cu, int n, int nb, float dl,
                       int max_p, int order_mode, float* out_xyz, int* out_lens,
                       int* out_total, void* ws, size_t ws_bytes, void* stream);

/* ---- a1 with attributes: features averaged, labels voted per voxel -----------
 * Replaces grid_subsampling.subsample_batch(points, batches, features=, classes=, sampleDl=, max_p=)
 * (cpp_subsampling/wrapper.cpp:62-82, :199-206 -> grid_subsampling.cpp:109 batch_grid_subsampling), called from
 * models/backbone_kpconv/kpconv.py:187-214.
 *   Points.   out_xyz, out_lens, out_total, the row order in both order modes, the max_p cut and the -1 code are bit
 *             for bit what spr_grid_subsample gives for the same arguments; the attribute rows follow the same row
 *             order and the same cut (grid_subsampling.cpp:181-204).
 *   Features. feat [n, fdim] f32 -> out_feat [n, fdim] f32, first *out_total rows valid.  Per voxel and column: the
 *             float32 sum of the voxel's points in original point order, starting from +0 (grid_subsampling.h:46,
 *             :59), then ONE IEEE division by (float)count (grid_subsampling.cpp:90-94) -- not the multiplication by
 *             (float)(1.0 / count) of the barycentre (:87).  No reassociation, no contraction.
 *   Labels.   lab [n, ldim] i32 -> out_lab [n, ldim] i32: per voxel and column the label with the largest count
 *             (grid_subsampling.h:50, :69; grid_subsampling.cpp:99-101).  Any int32 is a label; there is no cap on
 *             the number of distinct labels in a voxel.
 *   Ties.     max_element returns the FIRST maximum in the iteration order of the std::unordered_map<int, int> that
 *             received the voxel's labels in point order (grid_subsampling.cpp:100-101).  That order is a list rule:
 *             hash = the label sign-extended to size_t, bucket = hash % bucket_count; the bucket count grows
 *             1 -> 13 -> 29 -> 59 -> 127 -> ... when the 1st, 14th, 30th, 60th, 128th ... distinct label arrives (the
 *             schedule is measured on a real std::unordered_map<int, int> at run time, not tabulated); a new label
 *             whose bucket is empty goes to the front of the list, otherwise directly in front of the first list
 *             element of its bucket; a growth re-inserts the old list, front to back, by the same rule under the
 *             new bucket count.
 *   Arguments. fdim == 0: feat and out_feat are NULL (not read, not written); likewise ldim.  Both 0 is the plain
 *             call.  A negative dimension, or a NULL where the dimension is positive, is refused, status 2, before
 *             anything is enqueued; so is a workspace below spr_grid_subsample_attrs_workspace_size(n, nb, fdim,
 *             ldim), which is never below spr_grid_subsample_workspace_bytes(n, nb) and does not depend on fdim.
 *   ldim > 1 with nb > 1.  The reference slices the class vector of cloud b wrongly there
 *             (grid_subsampling.cpp:157-158: the slice ends at sum_b + len * ldim instead of (sum_b + len) * ldim),
 *             so for every cloud after the first the range is too short and can end before it begins, an invalid
 *             iterator pair for the vector constructor: undefined behaviour, nothing to reproduce.  This
 *             library applies the single-cloud rule to every cloud, with lab row i belonging to point i.  It is
 *             compared against the reference only for ldim == 1 or nb == 1.
 */
size_t spr_grid_subsample_attrs_workspace_size(int n, int nb, int fdim, int ldim);
int spr_grid_subsample_attrs(const float* xyz, const int* cu, int n, int nb, float dl, int max_p, int order_mode,
                             const float* feat, int fdim, const int* lab, int ldim, float* out_xyz, float* out_feat,
                             int* out_lab, int* out_lens, int* out_total, void* ws, size_t ws_bytes, void* stream);

/* ---- voxel pre-downsampling, one point per voxel ------------
 * Replaces voxel_down_sample of the KITTI loader (data_loaders/kitti_pred.py:12-14,
 * :203-204 -> kiss_icp): voxel = trunc(p / voxel_size) per axis in float64, the first point of
 * every voxel is kept.  out_idx [n] i32: the first out_count[0] entries = kept
 * original indices, ascending; out_count[0] = -1 when a coordinate exceeds 2^20 voxels.
 */
size_t spr_voxel_downsample_workspace_bytes(int n);
int spr_voxel_downsample(const float* xyz, int n, double voxel_size, int* out_idx,
                         int* out_count, void* ws, size_t ws_bytes, void* stream);

/* ---- raw KITTI scans of a whole batch -> the forward's clouds, one call ----------
 * Replaces the point path of KittiDataset.__getitem__ (data_loaders/kitti_pred.py:203-230) for every scan
 * of a batch: voxel_down_sample(xyz, voxel_size), the crop to crop_radius, the ground cut.  Per cloud b
 *   kept  = the first point (lowest index) of every voxel, voxel = trunc((double)p / voxel_size) per axis
 *           (spr_voxel_downsample's arithmetic);
 *   kept &= crop_radius <= 0 or sqrt(x*x + y*y) <= crop_radius   (float64, every operation rounded once);
 *   kept &= !remove_ground  or z > -1.0                           (strict)
 * in the loader's order: the masks act on the filter's output, so a voxel whose first point is masked yields
 * nothing (not its second point).  No sort: a per-cloud open-addressing table of point indices, five launches
 * and one memset for the whole batch, nothing read back.
 *   pts     [n, stride] f32, stride 3 or 4 (4: np.fromfile(...).reshape(-1, 4) as it is; the 4th column is
 *           never read)            cu [nb+1] i32 (device), every cloud at least one point
 *   out_xyz [n,3] f32, out_idx [n] i32: the first m rows are valid, m = out_cu[nb].  out_idx = the kept point's
 *           index inside its own cloud; ascending inside a cloud, clouds in input order
 *   out_cu  [nb+1] i32: cloud boundaries of the output (a cloud may come out empty)
 *   status  [1] i32: 0, or one of SPR_PREPARE_* (the outputs are then meaningless)
 *   scratch int32 [scratch_len], scratch_len >= spr_prepare_scans_scratch_len(n, nb) (a count of ints, not
 *           bytes); a shorter one is refused, status 2, before anything is enqueued.  n <= 2^31 - 1025.
 */
#define SPR_PREPARE_RANGE (-1)      /* a coordinate is not finite or not inside +-2^20 voxels (|p / voxel| < 2^20) */
#define SPR_PREPARE_PROBE (-2)      /* a point found no slot in its cloud's table region (cannot happen: load <= 1/2) */
#define SPR_PREPARE_BAD_LAYOUT (-3) /* cu is not an ascending prefix from 0 to n */
size_t spr_prepare_scans_scratch_len(int n, int nb);
int spr_prepare_scans(const float* pts, int stride, const int* cu, int n, int nb, double voxel_size,
                      double crop_radius, int remove_ground, int* scratch, size_t scratch_len,
                      float* out_xyz, int* out_idx, int* out_cu, int* status, void* stream);

/* ---- a2: batched fixed-radius neighbours ---------------------------------
 * Replaces radius_neighbors.batch_query(queries, supports, q_batches,
 * s_batches, radius=) (cpp_wrappers/cpp_neighbors/wrapper.cpp:58-75 ->
 * neighbors/neighbors.cpp:211 batch_nanoflann_neighbors) plus the
 * [:, :max_neighbors] slice of kpconv.py:258-262.
 * Rows: supports of the same cloud with d2 < r*r (float32, exact reference
 * arithmetic), ascending (d2, index), global indices, padded with ns.
 *   out_idx [nq, limit] i32, 1 <= limit <= 128; max_count [1] i32 device = untruncated max row
 *   count (the reference's row width); the caller may slice to
 *   min(max_count, limit).
 * algo 0: dense per-cloud cell table (fast; *max_count = -2 if the clouds'
 *   bounding boxes need more cells than the table holds -> retry with algo 1);
 * algo 1: sorted cell keys + binary search (no geometry limit besides 8191
 *   cells per axis, *max_count = -1).  Results are identical.
 * select: the rule that cuts a row with more than `limit` supports in range.
 *   SPR_SELECT_NEAREST keeps the `limit` nearest as described above (the
 *   reference's CPU Preprocessor).  SPR_SELECT_INDEX keeps the `limit` LOWEST
 *   support indices in range, ascending, padded with ns: the rows of the
 *   reference's PreprocessorGPU (batch_neighbors_kpconv_gpu, kpconv.py:265-292
 *   -> pytorch3d.ops.ball_query, the first K supports in index order).  The
 *   candidates are the same under both rules -- the same float32 d2, the same
 *   strict d2 < r*r -- and so is *max_count (the untruncated count, with its
 *   -1 / -2 codes); rows with at most `limit` supports in range hold the same
 *   set under both.  Any other value is an error.  Both algos and every algo
 *   of spr_radius_table_query give identical rows under either rule.
 */
size_t spr_radius_neighbors_workspace_bytes(int nq, int ns, int nb);
int spr_radius_neighbors(const float* q_xyz, const int* q_cu, int nq,
                         const float* s_xyz, const int* s_cu, int ns, int nb,
                         float radius, int limit, int algo, int select, int* out_idx,
                         int* max_count, void* ws, size_t ws_bytes, void* stream);

/* Cell table of spr_radius_neighbors (algo 0) as an object: built once per (supports, radius),
 * queried several times -- the pyramid runs the conv search, the pool search and the previous
 * level's up-sampling search against the same supports with the same radius (kpconv.py:352,
 * :377, :384).  Rows are those of spr_radius_neighbors, entry for entry.
 *   table: spr_radius_table_bytes(ns, nb) bytes, 256-byte aligned, owned by the caller;
 *   self != 0: the queries are the table's supports (same array and cu) -> cell-order walk;
 *   slot in [0, spr_radius_table_slots()): one per query call against a build (its max row count);
 *   *max_count as in spr_radius_neighbors (-2: geometry too large for the table -> algo 1);
 *   algo of spr_radius_table_query = the K-nearest selection -- 0: one thread per query (cell scan into a scratch
 *   row + rank sort in registers; cheaper for sparse rows), 1: one wave per query (one pass over the coalesced
 *   record runs, the row kept sorted in the wave's registers, no scratch, no sort kernel; faster when more
 *   supports lie in range than `limit`: LiDAR-shaped clouds), -1: the library's choice.  Identical rows.
 *   select as in spr_radius_neighbors; one table serves queries under either rule.
 */
size_t spr_radius_table_bytes(int ns, int nb);
size_t spr_radius_table_build_workspace_bytes(int ns, int nb);
size_t spr_radius_table_query_workspace_bytes(int nq);
int spr_radius_table_slots(void);
int spr_radius_table_build(const float* s_xyz, const int* s_cu, int ns, int nb, float radius,
                           void* table, size_t table_bytes, void* ws, size_t ws_bytes, void* stream);
int spr_radius_table_query(const float* q_xyz, const int* q_cu, int nq, int self, int ns, int nb,
                           float radius, int limit, int slot, const void* table, int* out_idx,
                           int* max_count, int algo, int select, void* ws, size_t ws_bytes, void* stream);

/* Count-only query against a built cell table: what calibrate_neighbors (kpconv.py:714-747 of the reference) needs
 * of a neighbour matrix with unbounded rows, without the matrix.  Per query, the number of supports of the same
 * cloud with d2 < r*r: exactly the candidates of spr_radius_table_query (same float32 d2, same strict <, same
 * 27 cells, same cell-order walk when self != 0), uncut -- no ceiling of 128 and none of hist_n.
 *   counts [nq] i32 or NULL: counts[i] = the count of query i;
 *   hist [nb, hist_n] i32 or NULL, 1 <= hist_n <= 4096: hist[c * hist_n + k] += the number of queries of cloud c
 *     whose count is exactly k, for k < hist_n; a query with hist_n or more supports in range is not binned (what
 *     np.bincount(c, minlength=hist_n)[:hist_n] makes of a row clipped at hist_n columns).  Added to, not
 *     overwritten: the caller zeroes it.  The row of a cloud without queries is not touched;
 *   status [1] i32 device: 0 fine, -1 / -2 the table's error codes as spr_radius_table_query reports them in
 *     *max_count (extent / radius beyond 8191 cells per axis; geometry too large for the table) -- counts and hist
 *     are then left as they were.
 * No workspace and no result slot of the table.  Arguments are checked on the host before the launch.
 */
int spr_radius_table_count(const float* q_xyz, const int* q_cu, int nq, int self, int ns, int nb,
                           float radius, const void* table, int* counts, int* hist, int hist_n,
                           int* status, void* stream);

/* ---- a2: neighbour ties in the reference's order ---------------------------------
 * The rows above order an equal-d2 run by index.  batch_nanoflann_neighbors (neighbors.cpp:211-332) orders it by the
 * kd-tree's visit order passed through an unstable std::sort (nanoflann.hpp:1279-1289): a deterministic function of
 * the cloud's supports, in cloud order, and of the query.  These entry points restate that function (nanoflann's tree
 * build with leaf size 10, its radius search with eps 0, libstdc++'s introsort on the distance alone; csrc/tie_order.h)
 * and rewrite, in place, the rows of a SPR_SELECT_NEAREST matrix in which an equal-d2 run touches the kept columns --
 * two kept entries with the same d2, or the last kept entry of a row cut at `width` and an entry behind the cut.
 * Afterwards the matrix equals the reference's, cut to its first `width` columns (kpconv.py:259-260), index for index.
 * Every other row keeps its bits.
 *   tree: spr_kdtree_replay_size(ns, nb) bytes, 256-byte aligned, owned by the caller; built once per support set
 *     (it does not depend on the radius) by spr_kdtree_replay_build, one wave per cloud.  Its first int32 is the depth
 *     of the deepest cloud's tree (nodes on the longest root-to-leaf path) once the build has run: the caller reads
 *     it and passes it as `depth`, which sizes the walk stacks;
 *   nbr [nq, stride] i32: the matrix as spr_radius_neighbors / spr_radius_table_query wrote it; width <= stride: the
 *     kept columns, min(max_count, limit); max_count: the search's untruncated widest row, which sizes a row's
 *     scratch;
 *   status [4] i32 device, written by every call: [0] rows_fixed, the rows rewritten; [1] set_mismatch, rows whose
 *     replayed neighbours are not the row's (left as they were; never expected); [2] rows whose replay did not fit
 *     max_count or depth (left as they were); [3] != 0: the tree is not one of these supports, failed to build, or is
 *     deeper than `depth` -- decided before any row is touched, and no row is.
 * A workspace smaller than the query's is refused before anything is enqueued.  The two size queries end in _size,
 * not _bytes: the workspace's is not monotone in max_count or depth (the fix-up runs fewer lanes, each with its own
 * stack and scratch, as a lane's share grows), which every *_bytes query of this header is.  spr_tie_order_host is the same
 * function on host memory (tree included; status on the host), spr_std_sort_replay_host the sort alone: perm_host
 * [n] = the order std::sort leaves n pairs (i, keys_host[i]) in when it compares keys only, *heap_ranges_host = the
 * ranges that exhausted the depth limit and were heap-sorted.
 */
size_t spr_kdtree_replay_size(int ns, int nb);
int spr_kdtree_replay_build(const float* s_xyz, const int* s_cu, int ns, int nb, void* tree, size_t tree_bytes,
                            void* stream);
size_t spr_tie_order_workspace_size(int nq, int max_count, int depth);
int spr_tie_order(const float* q_xyz, const int* q_cu, int nq, const float* s_xyz, const int* s_cu, int ns, int nb,
                  float radius, const void* tree, int depth, int* nbr, int stride, int width, int max_count,
                  int* status, void* ws, size_t ws_bytes, void* stream);
int spr_tie_order_host(const float* q_xyz_host, const int* q_cu_host, int nq, const float* s_xyz_host,
                       const int* s_cu_host, int ns, int nb, float radius, int* nbr_host, int stride, int width,
                       int max_count, int* status_host);
int spr_std_sort_replay_host(const float* keys_host, int n, int* perm_host, int* heap_ranges_host);

/* ---- 8f-5: ground-truth overlap masks and mutual correspondences ---------------
 * Replaces compute_overlap(src, tgt, search_voxel_size) (utils/pointcloud.py:8-65: one Open3D kd-tree radius query
 * per point), called per pair by the loaders (data_loaders/threedmatch.py:78-84) and by
 * data_processing/compute_overlap_3dmatch.py / compute_overlap_kitti.py.  One call labels all nb pairs, both
 * directions.  Contract (float64 on the exactly converted float32 inputs, one rounding per operation):
 *   s'_i = ((R0 x + R1 y) + R2 z) + t per output coordinate, pose [nb,3,4] f32 maps src -> tgt;
 *   d2(a, b) = ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2;
 *   src_corr[i] = the LOCAL target index j minimising (d2(s'_i, tgt_j), j) if that d2 < radius * radius (strict),
 *   else -1; tgt_corr[j] likewise over the transformed sources; masks = corr >= 0;
 *   corr [2, ns] i32: the mutual pairs (i, src_corr[i]) with src_corr[i] > 0 -- the reference's `> 0`
 *   (utils/pointcloud.py:57-58) drops a source whose mutual partner is target 0 -- and tgt_corr[src_corr[i]] == i,
 *   local indices, ascending i; pair c owns columns [src_cu[c], src_cu[c] + corr_count[c]) of both rows.
 * Outputs are identical to a float64 evaluation of these rules, whatever the batch composition.  Empty clouds and
 * clouds that do not overlap are legal (all -1).  Geometry never overflows the cell table (a cloud whose box needs
 * more than 16 n + 4096 cells gets coarser cells, same result); non-finite coordinates or poses give
 * corr_count[c] = -1 for every pair.
 *   src_xyz [ns,3] f32, src_cu [nb+1] i32, tgt_xyz [nt,3] f32, tgt_cu [nb+1] i32
 *   src_corr [ns] i32, tgt_corr [nt] i32, src_mask [ns] u8, tgt_mask [nt] u8, corr [2,ns] i32, corr_count [nb] i32
 */
size_t spr_gt_overlap_workspace_bytes(int ns, int nt, int nb);
int spr_gt_overlap(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz, const int* tgt_cu,
                   int nt, const float* pose, int nb, double radius, int* src_corr, int* tgt_corr,
                   unsigned char* src_mask, unsigned char* tgt_mask, int* corr, int* corr_count, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- 8f-6: training augmentation (perturb, jitter, shuffle, swap) -----------------
 * Replaces the per-pair CPU chain RigidPerturb -> Jitter -> ShufflePoints -> RandomSwap of the 3DMatch and KITTI
 * training loaders (data_loaders/transforms.py:15-179, composed in data_loaders/__init__.py:17-54).  One call
 * augments all nb pairs.  The reference draws from the global numpy / random / torch generators; here every draw is a
 * pure function of (seed, pair_key, side, element, stream tag): a pair is augmented identically whatever batch,
 * position, grid or rank it lands in.
 *
 * Draw contract.  Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85):
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (element, q & 0xffffffff, tag, q >> 32)  with q = 2 * pair_key + side (pair_key < 2^63; side 0 = source,
 *             1 = target; pair decisions use side 0) -- i.e. (element, 2 pair_key + side, tag, 0) for keys below 2^31
 *   tag     = 0 pair decisions, 1 jitter noise (element = ORIGINAL local point index), 2 shuffle keys (same)
 *   uniform u(w) = ((w >> 9) + 0.5) * 2^-23, in (0, 1), exact in float32 and float64 (24 significant bits)
 *   normal  from two words (a, b): r = sqrt(-2 ln u(a)), (r cos(2 pi u(b)), r sin(2 pi u(b))).
 * Jitter noise is float32 on the device: r = sqrtf(-2.f * logf(u(a))), angle = 6.2831855f * u(b), sincosf -- the
 * accurate library functions, one rounding per operation.  Point i gets, from the four words w0..w3 of its tag-1
 * block: (r(w0) cos(w1), r(w0) sin(w1), r(w2) cos(w3)).  Its shuffle key is word 0 of its tag-2 block.
 * Pair decisions are float64 on the host, from the tag-0 blocks of elements 0, 1, 2 (words e.w):
 *   perturb the source iff u(0.0) > 0.5, else the target; swap iff u(0.1) > 0.5   (random.random() > 0.5)
 *   SPR_AUG_SMALL (SE3.sample_small, std = 0.1): axis = (s cos phi, s sin phi, z) with z = 2 u(1.0) - 1,
 *     s = sqrt(1 - z^2), phi = 2 pi u(1.1); angle = n(1.2, 1.3).cos * std * pi / sqrt(3); rotation by Rodrigues'
 *     formula; translation = (n(2.0, 2.1).cos, n(2.0, 2.1).sin, n(2.2, 2.3).cos) * std / sqrt(3)
 *   SPR_AUG_LARGE: Euler angles (z, y, x) = 2 pi (u(1.0), u(1.1), u(1.2)), R = Rx Ry Rz (the extrinsic
 *     'zyx' of scipy.spatial.transform.Rotation.from_euler); translation = -4 + 8 (u(2.0), u(2.1), u(2.2))
 *   SPR_AUG_NONE: identity (and spr_augment_pairs applies no perturbation whatever it is handed).
 *   The [3,4] result is rounded to float32.
 *
 * spr_philox4x32_host: one block on the host (the known-answer entry).
 * spr_augment_draw: the decisions of nb pairs into HOST arrays (perturb_src_host [nb] u8, swap_host [nb] u8,
 *   perturb_host [nb,3,4] f32; each may be NULL) and, when `noise` / `keys` are given, the device buffers
 *   noise [ns+nt,3] f32 and keys [ns+nt] u32 of a batch with the given src_cu / tgt_cu and DEVICE pair_key [nb] u64,
 *   in the stacked order [all sources, all targets].  These are the values spr_augment_pairs generates inline when it
 *   is handed NULL for them: inline and explicit agree bit for bit.
 *
 * spr_augment_pairs.  Contract (float64 on the exactly converted float32 inputs, one rounding per operation, sums of
 * three products as ((a0 b0 + a1 b1) + a2 b2); every named intermediate is rounded to float32):
 *   cat(A, B) = [A_R B_R | A_R B_t + A_t],  inv(A) = [A_R^T | -(A_R^T A_t)]
 *   centroid c = f32(sum_f64(points of the perturbed cloud) / n)             (mode SMALL only; n = 0 -> 0)
 *   P' = f32([R | (R (-c)) + (t + c)])   (= C^-1 P C, C the translation by -c)   SMALL;   P' = P   LARGE
 *   pose' = f32(cat(pose, inv(P'))) when the source is perturbed, f32(cat(P', pose)) when the target is
 *   x' = f32(((R'0 x + R'1 y) + R'2 z) + t') for the points of the perturbed cloud, x' = x for the other
 *   x'' = x' + f32(noise * scale)   in float32, both clouds, noise indexed by the ORIGINAL point index
 *   shuffle: per cloud the stable ascending order of its 32-bit keys, cut to the first max_pts; masks are gathered
 *     with the points; perm = the original local index of every output point
 *   correspondences are remapped through the inverse permutation; those with an end cut away (or out of range) are
 *     dropped, the survivors keep their relative order
 *   swap: the pair's clouds, masks, permutations and correspondence rows change sides, pose_out = f32(inv(pose')).
 * flags [nb] u8: bit 0 = perturb the source (else the target), bit 1 = swap.  mode: SPR_AUG_*.
 * Output lengths are known to the caller: min(len, max_pts) per cloud, sides exchanged where the pair swaps;
 * out_src_cu / out_tgt_cu [nb+1] i32 are written on the device.  Only the number of surviving correspondences is data
 * dependent: pair c owns columns [corr_off[c], corr_off[c] + corr_count[c]) of both rows of corr [2, corr_stride]
 * (corr_off ascending, runs disjoint -- spr_gt_overlap's layout with corr_off = src_cu, corr_stride = ns) and the same
 * columns, from corr_off[c], of out_corr; out_corr_count [nb] i32.
 * status [nb] i32: 0, or 1 when the pair has a non-finite coordinate, pose or perturbation (its outputs are then
 * unspecified but every index is in range; other pairs are unaffected).
 * Empty clouds, SPR_AUG_NONE, scale = 0, max_pts above every length and pairs without correspondences are legal.
 *   src_xyz [ns,3] f32, tgt_xyz [nt,3] f32, src_cu / tgt_cu [nb+1] i32, pose [nb,3,4] f32, perturb [nb,3,4] f32,
 *   src_mask [ns] / tgt_mask [nt] u8 (both or neither; NULL: no masks, out masks untouched),
 *   corr NULL: no correspondences (corr_off, corr_count, out_corr, out_corr_count unused),
 *   noise / keys: NULL = generated inline from (seed, pair_key); pair_key [nb] u64 is then required,
 *   out_src_xyz / out_tgt_xyz [.,3] f32, out_*_mask u8 and out_*_perm i32 hold the sum of that side's output lengths
 *   (ns + nt rows always suffice); out_pose [nb,3,4] f32; out_corr [2,corr_stride] i32.
 */
#define SPR_AUG_NONE 0
#define SPR_AUG_SMALL 1
#define SPR_AUG_LARGE 2
int spr_philox4x32_host(const uint32_t* ctr_host, const uint32_t* key_host, uint32_t* out_host);
int spr_augment_draw(uint64_t seed, const uint64_t* pair_key_host, int nb, int mode, unsigned char* perturb_src_host,
                     unsigned char* swap_host, float* perturb_host, const uint64_t* pair_key, const int* src_cu,
                     int ns, const int* tgt_cu, int nt, float* noise, unsigned int* keys, void* stream);
size_t spr_augment_workspace_bytes(int ns, int nt, int nb, int corr_stride);
int spr_augment_pairs(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz, const int* tgt_cu,
                      int nt, const float* pose, int nb, const unsigned char* src_mask,
                      const unsigned char* tgt_mask, const int* corr, int corr_stride, const int* corr_off,
                      const int* corr_count, const float* perturb, const unsigned char* flags, int mode, float scale,
                      int max_pts, uint64_t seed, const uint64_t* pair_key, const float* noise,
                      const unsigned int* keys, float* out_src_xyz, float* out_tgt_xyz, int* out_src_cu,
                      int* out_tgt_cu, float* out_pose, unsigned char* out_src_mask, unsigned char* out_tgt_mask,
                      int* out_src_perm, int* out_tgt_perm, int* out_corr, int* out_corr_count, int* status, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- 8f-7: ModelNet training pairs (crop, transform, resample, jitter, shuffle) ------
 * Replaces the per-sample CPU chain SplitSourceRef -> RandomCrop(partial) -> RandomTransformSE3_euler(rot_mag,
 * trans_mag) -> Resampler(num_points) -> RandomJitter() -> ShufflePoints() of the reference's ModelNet loader
 * (data_loaders/modelnet.py:102-109, data_loaders/modelnet_transforms.py) for noise_type 'crop': one raw cloud in,
 * a partially overlapping (source, reference) pair with its pose, overlap masks and correspondences out.  One call
 * generates all nb pairs; every draw is a pure function of (seed, pair_key, side, element, stream tag).
 *
 * Draw contract.  Philox4x32-10, key, counter layout and u(w) of 8f-6, q = 2 * pair_key + side (side 0 = source,
 * 1 = reference cloud; pair-level draws use side 0 unless a side is named).  Words of a block: w0..w3.
 *   tag 16, host, float64 (libm acos / sin / cos):
 *     element 0 of side s: that side's crop direction (uniform_2_sphere): phi = 2 pi u(w0), z = 2 u(w1) - 1,
 *       theta = acos z, dir = (sin theta cos phi, sin theta sin phi, cos theta)
 *     element 1: angles (a_x, a_y, a_z) = ((u(w0..w2) * pi) * rot_mag) / 180
 *     element 2: translation t = -trans_mag + (2 * trans_mag) * u(w0..w2)
 *     R = (Rx Ry) Rz with the matrices of modelnet_transforms.py:342-351, every entry ((a0 b0 + a1 b1) + a2 b2);
 *     [R | t] is rounded to float32
 *   tag 17: the resample key of a point = w0 of the block whose element is the point's RAW local index
 *   tag 18: up-sampling extras: position n_kept + j takes the kept point floor(u(w0 of element j) * n_kept) (float64;
 *     the product is exact), the kept points counted in ascending raw order (the cropped cloud's own order)
 *   tag 19: jitter noise = the 8f-6 float32 normal triple of the block whose element is the RESAMPLED position
 *   tag 20: the shuffle key = w0 of the block whose element is the resampled position
 *
 * spr_modelnet_draw: the decisions of nb pairs into HOST arrays (dirs_host [nb,2,3] f64, transform_host [nb,3,4] f32;
 *   each may be NULL) and, when any of them is given, the device buffers of the per-point draws of a batch with the
 *   given cu and DEVICE pair_key [nb] u64: rkeys [2,n_total] u32 (tag 17), extra [2,nb*k] u32 (tag 18, the words w0),
 *   noise [2,nb*k,3] f32 (tag 19), skeys [2,nb*k] u32 (tag 20); first index = side, pair b owns entries from b*k.
 *   These are the values spr_modelnet_pairs generates inline when it is handed NULL for them: bit for bit.
 *
 * spr_modelnet_pairs.  Contract (float64 on the exactly converted float32 inputs, one rounding per operation, sums of
 * three products as ((a0 b0 + a1 b1) + a2 b2), no contraction; f32(.) = rounded to float32).  Cloud b = rows
 * [cu[b], cu[b+1]) of xyz, n points, local ("raw") indices 0..n-1; both sides start from the same n points.
 *   1 centre and project (per side): c = f32(S / n), S = the float64 sum of the cloud in this fixed order: partial
 *     p_t = x_t + x_(t+1024) + ... (ascending, t < 1024, absent terms skipped); inside every run of 64 consecutive
 *     partials six rounds p_t <- p_t + p_(t xor o), o = 32, 16, 8, 4, 2, 1; the 16 run sums added in ascending order
 *     from 0.  v = f32(x - c); d = dot3(v, dir).
 *   2 crop mask (RandomCrop.crop): p_keep = 1 keeps everything; p_keep = 0.5 keeps d > 0; otherwise numpy's 'linear'
 *     percentile: h = (n-1) * (q / 100), lo = floor(h), t = h - lo, a / b = the lo-th / min(lo+1, n-1)-th smallest d,
 *     thr = a + (b-a) t if t < 0.5 else b - (b-a) (1-t); keep d > thr.  q is the caller's float64 (1 - f32(p)) * 100
 *     evaluated as the reference does (30.000001907348633 for 0.7).
 *   3 a kept source point is "overlap" iff its raw index is kept on the reference side, and the other way round; the
 *     correspondences are the raw indices kept on both sides, in ascending raw order.
 *   4 transform, source only: x' = f32(dot3(R_i, x) + t_i);  pose = f32([R^T | -(R^T t)]) maps source -> reference.
 *   5 resample to k per side: the kept points in the stable ascending order of their tag-17 keys, cut to k; with
 *     n_kept < k all of them in that order, then the tag-18 extras.  A correspondence survives iff both its ends were
 *     selected; where a point occupies several positions it maps to the LARGEST one (numpy's repeated-index
 *     assignment).  Survivors keep their order.
 *   6 jitter, both sides: e = clamp(f32(noise * scale), -clip, clip) per component, x'' = f32(x' + e).
 *   7 shuffle, both sides: out[j] = resampled[perm[j]], perm = the stable ascending order of the tag-20 keys; overlap
 *     flags and raw indices are gathered with the points, correspondences go through the inverse permutation.
 * Outputs, k entries per pair and side, pair b from b*k: src_xyz / tgt_xyz [nb*k,3] f32, src_overlap / tgt_overlap
 * [nb*k] u8, src_index / tgt_index [nb*k] i32 (the raw local index of every output point), pose [nb,3,4] f32,
 * corr [2, nb*k] i32 (row 0 source, row 1 reference output indices; pair b owns columns [b*k, b*k + corr_count[b])),
 * corr_count [nb] i32 -- the only data-dependent size.
 * status [nb] i32: 0; 1 = a non-finite coordinate, transform or direction in that pair; 2 = a side keeps no point
 * after the crop (n <= 1, or every d equal); 3 = the cloud is longer than max_len_host or outside xyz.  A pair with a
 * non-zero status has zero points, flags and indices and no correspondences (its pose is still written for 2); other
 * pairs are unaffected.
 * max_len_host: an upper bound of the longest cloud, at most 8192; k in [1, 8192]; p_keep in (0, 1].  Violations are
 * refused on the host before any launch.  Ragged lengths and empty clouds are legal.
 *   xyz [n_total,3] f32, cu [nb+1] i32, transform [nb,3,4] f32, dirs [nb,2,3] f64, pair_key [nb] u64 (all device);
 *   rkeys / extra / noise / skeys: the explicit draw buffers above, each NULL = generated inline (pair_key required).
 */
int spr_modelnet_draw(uint64_t seed, const uint64_t* pair_key_host, int nb, double rot_mag, double trans_mag,
                      double* dirs_host, float* transform_host, const uint64_t* pair_key, const int* cu, int n_total,
                      int k, unsigned int* rkeys, unsigned int* extra, float* noise, unsigned int* skeys, void* stream);
size_t spr_modelnet_pairs_workspace_size(int n_total, int nb, int k);
int spr_modelnet_pairs(const float* xyz, const int* cu, int n_total, int nb, int max_len_host, float p_src, float p_tgt,
                       double q_src, double q_tgt, int k, float scale, float clip, const float* transform,
                       const double* dirs, uint64_t seed, const uint64_t* pair_key, const unsigned int* rkeys,
                       const unsigned int* extra, const float* noise, const unsigned int* skeys, float* src_xyz,
                       float* tgt_xyz, float* pose, unsigned char* src_overlap, unsigned char* tgt_overlap,
                       int* src_index, int* tgt_index, int* corr, int* corr_count, int* status, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- surface normals as per-point input features: estimate, gather + rotate -----------
 * Neither has a counterpart in the reference's hot path: its ModelNet files ship normals and its transform chain
 * carries and rotates them (data_loaders/modelnet_transforms.py:285-289); estimating them is left to the user there.
 *
 * spr_estimate_normals: PCA normals over a neighbour matrix the caller already has.
 *   xyz [n,3] f32 packed, cu [nb+1] i32; nbr [n, nbr_stride] i32, of which the first kmax columns are used.  Entries
 *   are global rows of xyz; an entry outside [0, n) is a shadow, may sit at any column and contributes nothing.  This
 *   is the matrix spr_radius_neighbors gives for queries = supports = xyz: it holds the point itself, and the kernel
 *   adds nothing of its own.  viewpoint [nb,3] f32 (one per cloud) or NULL; cu is read only with a viewpoint.
 *   normals [n,3] f32; curvature [n] f32 or NULL.  No workspace, no device-to-host read; n = 0 and kmax = 0 are legal.
 *   Contract (float64 on the exactly converted float32 inputs), per point i with m valid entries j:
 *     m < 3: normal (0, 0, 0), curvature 0.  Otherwise
 *     d_j = p_j - p_i,  mu = sum d_j / m,  C = sum (d_j - mu)(d_j - mu)^T / m,  eigenvalues l0 <= l1 <= l2 of C;
 *     n = the unit eigenvector of l0;  curvature = l0 / (l0 + l1 + l2), or 0 when the trace is 0.
 *   Sign of n: with a viewpoint v of the point's cloud, n is flipped when n . (v - p_i) < 0.  Without one, or when
 *     that product is exactly 0, it is flipped so that its component of largest magnitude is positive (the lowest
 *     index among equal magnitudes).
 *   The arithmetic is float32: the count and the nine moments sum d, sum d d^T relative to the query point (so a cloud
 *   far from the origin is as well conditioned as one at it), C = E[d d^T] - mu mu^T, and a cyclic Jacobi on C / trace
 *   in registers.  With u = 2^-24 the result is an exact eigenvector of a covariance within (kmax + 8) u |C| of C:
 *     n^T C n <= l0 + 2 (kmax + 8) u l2,   |n x n_ref| <= (kmax + 8) u l2 / (l1 - l0),   | |n| - 1 | <= 4 * 2^-23,
 *     |curvature - ref| <= (kmax + 8) u.
 *   Where l0 = l1 (or all of C is 0) the eigenvector is not unique and any unit vector of the eigenspace is returned.
 *   The sums are taken in a fixed order: results are reproducible bit for bit.
 *
 * spr_feats_gather_rotate: out[r, :] = feats[rows[r], :], with every listed column triple rotated.
 *   feats [n_in, c] f32; rows [n_out] i32, global rows of feats (a row outside [0, n_in) gives zeros); cu_out [nb+1]
 *   i32 over the OUTPUT rows; rot [nb,3,3] f32 row-major, one rotation per output cloud (identity where none);
 *   dir_cols_host [n_dir] int, n_dir <= 4: the first column of every direction triple.  A triple running past c,
 *   overlapping triples and n_dir > 4 are refused, status 2.  out [n_out, c] f32.  cu_out and rot are read only when
 *   n_dir > 0.  n_out = 0 and empty clouds are legal.
 *   Scalar columns are copied.  A triple (x, y, z) of a row of cloud b becomes, for k = 0, 1, 2,
 *     f32((R_k0 x + R_k1 y) + R_k2 z),  R = rot[b],
 *   evaluated in float64 with one rounding per operation (the convention of 8f-6): a float64 restatement is bit-equal.
 *   Directions are not renormalised.
 */
int spr_estimate_normals(const float* xyz, const int* cu, int n, int nb, const int* nbr, int nbr_stride, int kmax,
                         const float* viewpoint, float* normals, float* curvature, void* stream);
int spr_feats_gather_rotate(const float* feats, int n_in, int c, const int* rows, int n_out, const int* cu_out, int nb,
                            const float* rot, const int* dir_cols_host, int n_dir, float* out, void* stream);

/* ---- a4: KPConv forward ---------------------------------------------------
 * Replaces KPConv.forward(q_pts, s_pts, neighb_inds, x)
 * (models/backbone_kpconv/kpconv_blocks.py:269-414; rigid kernel, linear
 * influence, 'sum' aggregation -- the only mode any shipped config selects).
 *   nbr [nq, nbr_stride] i32, first `kmax` columns used, shadow index = ns
 *   x [ns, cin]  weights [n_kp, cin, cout]  kernel_points [n_kp, 3]
 *   out [nq, cout]
 * rows_sorted != 0 promises that shadow entries only trail valid ones (true
 * for spr_radius_neighbors output) and enables early exit.
 * impl: 0 = default (ring kernel for 32/64-channel inputs, streamed MFMA tile kernel otherwise),
 *       1 = simple reference kernel, 2 = the streamed MFMA tile kernel for every MFMA shape (A/B).
 * x_range / w_range: operand ranges of x and the weights as in spr_linear (NULL = measured here).
 * plan / wplanes: the static inputs of the ring KPConv (csrc/kpconv.hip, k_kpconv_ring), hoisted out of the
 * per-call path (NULL = built per call).  Both are pure functions of their arguments; callers cache them per
 * neighbour matrix / per weight version (ops.py does).  The reference recomputes everything per call
 * (kpconv_blocks.py:269-414); these have no counterpart there.
 *   spr_kpconv_plan: tile descriptors of a neighbour matrix -- tiles of 16 queries (in `order` if
 *     given: a permutation of [0, nq), e.g. a spatial order; NULL = natural order), the 16 queries of
 *     a tile dealt to the eight waves by live neighbour-block count.  The plan depends on
 *     (nbr contents, nq, ns, nbr_stride, kmax, rows_sorted, order) only.
 *   spr_kpconv_prep_weights: the [15, cin, cout] weights as range-scaled split-fp16 planes in
 *     MFMA-fragment order; w_range = spr_absmax partials of the same weights (required, and the same
 *     w_range goes to spr_kpconv_fwd with the planes).
 */
size_t spr_kpconv_workspace_bytes(int nq, int ns, int cin, int cout);
size_t spr_kpconv_plan_bytes(int nq);
int spr_kpconv_plan(const int* nbr, int nq, int ns, int nbr_stride, int kmax, int rows_sorted,
                    const int* order, void* plan, size_t plan_bytes, void* stream);
size_t spr_kpconv_wplanes_bytes(int cin, int cout);
int spr_kpconv_prep_weights(const float* weights, int n_kp, int cin, int cout, const float* w_range,
                            int w_range_n, void* wplanes, size_t wplanes_bytes, void* stream);
int spr_kpconv_fwd(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                   int nbr_stride, int kmax, int rows_sorted, const float* x, int cin,
                   const float* weights, int cout, const float* kernel_points, int n_kp,
                   float kp_extent, float* out, int impl, const float* x_range, int x_range_n,
                   const float* w_range, int w_range_n, const void* plan, const void* wplanes,
                   void* ws, size_t ws_bytes, void* stream);

/* KPConv in the reference's other modes (kpconv_blocks.py:361-385; rigid kernel points; csrc/kpconv_modes.hip):
 *   influence    SPR_KP_CONSTANT  w = 1
 *                SPR_KP_LINEAR    w = max(0, 1 - sqrt(d2) / kp_extent)                  (spr_kpconv_fwd's rule)
 *                SPR_KP_GAUSSIAN  w = exp(-d2 / (2 sigma^2 + 1e-9)), sigma = 0.3 kp_extent   (no cut-off)
 *   aggregation  SPR_KP_SUM       every kernel point weighs on a neighbour
 *                SPR_KP_CLOSEST   only p = argmin_p d2 does (the lowest p on a tie, torch.argmin)
 * with d2[n,k,p] = |s[nbr[n,k]] - q[n] - kernel_points[p]|^2 in float32.  An index outside [0, ns) contributes nothing
 * and is not counted; the output is divided by max(1, #{k : sum_c x[nbr[n,k],c] > 0}), counted from the flags
 * spr_kpconv_fwd counts from (one summation order).  An unknown influence / aggregation returns status 2.
 * linear / sum is valid here and agrees with spr_kpconv_fwd to rounding, not to the bit (another kernel, another order).
 * spr_kpconv_modes_fwd takes spr_kpconv_fwd's arguments without rows_sorted and plan (the kernel compacts each row
 *   itself and has no tile plan); impl: 0 = fused tile kernel for 15 kernel points with cin, cout multiples of 32 and
 *   cout <= 256, one thread per output element otherwise; 1 = the latter for every shape.  wplanes:
 *   spr_kpconv_prep_weights of THESE weights with THIS w_range, as for spr_kpconv_fwd (NULL = built here, per call).
 * spr_kpconv_modes_weighted_features / spr_kpconv_modes_bwd_dx: spr_kpconv_weighted_features / spr_kpconv_bwd_dx in
 *   the given mode (declared with the backward below for the default mode): wf [nq, n_kp * cin] un-normalised and
 *   cnt [nq] = max(1, count); dx [ns, cin] fully written, 64-bit fixed-point sums (bitwise reproducible),
 *   ws: spr_scatter_workspace_bytes(ns, cin).  The influences and the arg-min are constants of the backward (kernel
 *   points are not trained); with two GEMMs in between = the KPConv backward.  n_kp <= 16. */
#define SPR_KP_CONSTANT 0
#define SPR_KP_LINEAR 1
#define SPR_KP_GAUSSIAN 2
#define SPR_KP_SUM 0
#define SPR_KP_CLOSEST 1
size_t spr_kpconv_modes_workspace_size(int nq, int ns, int cin, int cout);
int spr_kpconv_modes_fwd(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride,
                         int kmax, const float* x, int cin, const float* weights, int cout,
                         const float* kernel_points, int n_kp, float kp_extent, int influence, int aggregation,
                         float* out, int impl, const float* x_range, int x_range_n, const float* w_range,
                         int w_range_n, const void* wplanes, void* ws, size_t ws_bytes, void* stream);
size_t spr_kpconv_modes_weighted_features_workspace_size(int ns);
int spr_kpconv_modes_weighted_features(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                       int nbr_stride, int kmax, const float* x, int cin, const float* kernel_points,
                                       int n_kp, float kp_extent, int influence, int aggregation, float* wf,
                                       float* cnt, void* ws, size_t ws_bytes, void* stream);
int spr_kpconv_modes_bwd_dx(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride,
                            int kmax, int cin, const float* kernel_points, int n_kp, float kp_extent, int influence,
                            int aggregation, const float* dwf, const float* dwf_range, int dwf_range_n, float* dx,
                            void* ws, size_t ws_bytes, void* stream);

/* Deformable / modulated KPConv, linear influence and sum aggregation (kpconv_blocks.py:309-412 with deformable=True;
 * csrc/kpconv_deform.hip).  offset_features [nq, of_stride >= (3 + modulated) n_kp] is the caller's offset convolution
 * plus bias.  With K = n_kp, e = kp_extent, y = s[nbr[n,k]] - q[n], all float32:
 *   D[n,p,:] = kernel_points[p] + e of[n, 3p:3p+3];   m[n,p] = 2 sigmoid(of[n, 3K+p]) when modulated, else 1
 *   d2[n,k,p] = |y - D[n,p]|^2;   in_range[n,k] = any_p d2 < e^2 (an index outside [0, ns) is never in range)
 *   h = max(0, 1 - sqrt(d2) / e) for in-range neighbours, 0 otherwise
 *   out[n,:] = sum_p (m[n,p] sum_k h[n,k,p] x[nbr[n,k],:]) W[p] / max(1, #{k : in_range[n,k], sum_c x[nbr[n,k],c] > 0})
 *   (the rigid kernels count every valid neighbour; the flags are spr_kpconv_fwd's, one summation order)
 *   min_d2 [nq, K] (optional, NULL = not wanted) = min_k d2[n,k,p], a shadow entry taking part as (1e6, 1e6, 1e6).
 * spr_kpconv_deform_fwd: spr_kpconv_modes_fwd's arguments without the mode pair; impl and wplanes as there (tile kernel
 *   for 15 kernel points, cin and cout multiples of 32, cout <= 256).  n_kp <= 16 everywhere.
 * The backward, with dwfm = (dout / cnt) W_flat^T [nq, K cin] from two GEMMs of the caller:
 *   spr_kpconv_deform_weighted_features: wf [nq, K cin] UNmodulated and un-normalised, cnt [nq] = max(1, count) as above
 *   spr_kpconv_deform_bwd_dx: dx[nbr[n,k], c] += sum_p h m dwfm[n,p,c]; dx [ns, cin] fully written, 64-bit fixed-point
 *     sums (bitwise reproducible); ws: spr_scatter_workspace_bytes(ns, cin)
 *   spr_kpconv_deform_bwd_offsets: d_offset_features [nq, (3 + modulated) K] contiguous, every element written, sums in a
 *     fixed order (bitwise reproducible), no workspace; with g[n,k,p] = sum_c dwfm[n,p,c] x[nbr[n,k],c]:
 *       d of[n, 3p:3p+3] = e m sum_k g (y - D[n,p]) / (sqrt(d2) e) over items with 0 < sqrt(d2) < e
 *       d of[n, 3K+p]    = (sum_k h g) 2 s (1 - s),  s = sigmoid(of[n, 3K+p])
 *     An item with d2 == 0 contributes 0 (the reference's sqrt yields NaN there).  No gradient reaches the points or
 *     the count. */
size_t spr_kpconv_deform_workspace_size(int nq, int ns, int cin, int cout);
int spr_kpconv_deform_fwd(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride,
                          int kmax, const float* x, int cin, const float* weights, int cout,
                          const float* kernel_points, int n_kp, float kp_extent, const float* offset_features,
                          int of_stride, int modulated, float* out, float* min_d2, int impl, const float* x_range,
                          int x_range_n, const float* w_range, int w_range_n, const void* wplanes, void* ws,
                          size_t ws_bytes, void* stream);
size_t spr_kpconv_deform_weighted_features_workspace_size(int ns);
int spr_kpconv_deform_weighted_features(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                        int nbr_stride, int kmax, const float* x, int cin, const float* kernel_points,
                                        int n_kp, float kp_extent, const float* offset_features, int of_stride,
                                        float* wf, float* cnt, void* ws, size_t ws_bytes, void* stream);
int spr_kpconv_deform_bwd_dx(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride,
                             int kmax, int cin, const float* kernel_points, int n_kp, float kp_extent,
                             const float* offset_features, int of_stride, int modulated, const float* dwfm,
                             const float* dwfm_range, int dwfm_range_n, float* dx, void* ws, size_t ws_bytes,
                             void* stream);
int spr_kpconv_deform_bwd_offsets(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                                  int nbr_stride, int kmax, const float* x, int cin, const float* kernel_points,
                                  int n_kp, float kp_extent, const float* offset_features, int of_stride,
                                  int modulated, const float* dwfm, float* d_offset_features, void* stream);

/* The regulariser of deformable KPConv (csrc/deform_reg.hip): KPConv's fitting loss (the squared distance from every
 * deformed kernel point to its nearest input point) and repulsive loss (a query's kernel points may not collapse onto
 * each other), value and gradient at the offset features in one launch.  Inputs as spr_kpconv_deform_fwd's;
 * R = repulse_extent (in units of e); K = n_kp <= 16:
 *   D[n,p]  = kernel_points[p] + e of[n, 3p:3p+3]            (float32, the arithmetic of min_d2 above)
 *   y[n,k]  = s[nbr[n,k]] - q[n]                             real entries only: an index outside [0, ns) is a shadow
 *   m[n,p]  = min over real k of |y[n,k] - D[n,p]|^2;  k* = the lowest column that attains it
 *             a row with no real entry: m[n,p] = 0 and no k*
 *   fit     = 1/(nq K) sum_{n,p} m[n,p] / e^2
 *   L       = D / e;  dist[n,i,j] = |L[n,i] - L[n,j]|
 *   rep     = 1/(nq K) sum_n sum_i sum_{j != i} min(dist[n,i,j] - R, 0)^2
 *   out[3]  = (2 fit + rep, fit, rep), float32; the sums are float64 per-workgroup partials (in ws) added in block
 *             order: no atomics, two runs give the same bits
 * d_offset_features (NULL = not wanted: nothing but the partials is stored): [nq, (3 + modulated) K] contiguous, every
 * element written.  In the repulsive term the OTHER kernel points are constants, as KPConv's authors detach them:
 *   d of[n, 3p:3p+3] = 1/(nq K) [4 (D[n,p] - y[n,k*]) / e + 2 sum_{j != p} min(dist[n,p,j] - R, 0) (L[n,p] - L[n,j]) / dist[n,p,j]]
 *   d of[n, 3K + p]  = 0                                     (modulation logits)
 * A pair with dist == 0 contributes 0 to the gradient (the authors' sqrt yields NaN there); a row with no real
 * neighbour contributes 0 to the fit term and to its gradient.
 * Deliberate deviation: KPConv's authors let a shadow entry take part in the minimum as the point (1e6, 1e6, 1e6).  For
 * a row that holds a real neighbour the two definitions agree (coordinates are far below 1e6); an all-shadow row would
 * add about 3e12 / e^2 to a mean of O(1) terms.  The pyramid never builds such a row (a pooled query lies within half a
 * cell diagonal of one of its own points).  min_d2 of spr_kpconv_deform_fwd keeps the far-point contract. */
size_t spr_deform_reg_workspace_size(int nq);
int spr_deform_reg(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride, int kmax,
                   const float* kernel_points, int n_kp, float kp_extent, const float* offset_features, int of_stride,
                   int modulated, float repulse_extent, float* out, float* d_offset_features, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- ICP for all pairs: point-to-point refinement of a pose, and its evaluation (fitness, inlier RMSE) -----------
 * The loop of Open3D's registration_icp with TransformationEstimationPointToPoint, which the reference's KITTI loader
 * runs on every ground-truth pose (data_loaders/kitti_pred.py:161-183: raw scans, threshold 0.2 m, 200 iterations),
 * for all nb pairs of a batch in one call; max_iter = 0 is a pure evaluation of pose_init.  Open3D is not available
 * here: parity with it is unpinned, the definition below is the contract.
 * Contract, per pair, in IEEE float64 on the exactly converted float32 inputs, one rounding per operation, no FMA:
 *   s'_i[k]  = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k]                  (T = [R | t], src -> tgt)
 *   d2(a, b) = ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2
 *   E(T), the evaluation under T:
 *     corr_i      = the LOCAL target index j minimising (d2(s'_i, tgt_j), j) if that d2 < max_dist * max_dist (strict),
 *                   else -1
 *     count       = #{corr_i >= 0}
 *     fitness     = count / n_src                                             (0 for an empty source)
 *     inlier_rmse = sqrt(sum of the matched d2 / count)                       (0 when count = 0)
 *   T_0 = pose_init; evaluate E(T_0); then for k = 0 .. max_iter - 1:
 *     U = the unweighted Kabsch solve of the pairs (s'_i, tgt_corr_i): R from the SVD of sum (a - mean a)(b - mean b)^T
 *         with the sign fix at det <= 0, t = mean b - R mean a -- the arithmetic of spr_weighted_procrustes kept in
 *         float64; count = 0 gives U = I
 *     T_{k+1} = U o T_k, composed in float64; evaluate E(T_{k+1})
 *     stop after this pass if |fitness_{k+1} - fitness_k| < rel_fitness and |rmse_{k+1} - rmse_k| < rel_rmse
 *   iterations = the number of steps k run; every output is that of the LAST evaluation.
 * One pass over the correspondences serves the evaluation of T_k and the solve for T_{k+1}: a call makes
 * iterations + 1 association passes per pair.  The order of the moment sums is the implementation's, fixed and a
 * function of the pair alone (per-block float64 partials added in block order, no floating-point atomics): every
 * output of a pair has the same bits whatever batch, position or neighbours it is called with, and run to run.  A
 * pair that has stopped is frozen: later passes of the call neither touch it nor do association work for it.
 * Empty sources and targets are legal (fitness 0, pose = pose_init).  status [nb] i32: 0, or -1 when the pair has a
 * non-finite coordinate or pose: pose = pose_init, fitness = rmse = 0, iterations = count = 0, corr = -1 for that
 * pair only.  Geometry never overflows the target's cell table (spr_gt_overlap's rule: a cloud whose box needs more
 * than 16 n + 4096 cells at edge max_dist (1 + 2^-8) gets coarser cells, same result).
 * The call reads one integer back from the device per four passes (none when max_iter < 4); a workspace below
 * spr_icp_pairs_workspace_size(ns, nt, nb) is refused before anything is enqueued.
 *   src_xyz [ns,3] f32, src_cu [nb+1] i32, tgt_xyz [nt,3] f32, tgt_cu [nb+1] i32, pose_init [nb,3,4] f64
 *   max_dist > 0, max_iter >= 0
 *   pose [nb,3,4] f32 (= pose64 rounded), pose64 [nb,3,4] f64, fitness [nb] f64, inlier_rmse [nb] f64,
 *   iterations [nb] i32, count [nb] i32, corr [ns] i32, status [nb] i32 */
size_t spr_icp_pairs_workspace_size(int ns, int nt, int nb);
int spr_icp_pairs(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz, const int* tgt_cu, int nt,
                  const double* pose_init, int nb, double max_dist, int max_iter, double rel_fitness, double rel_rmse,
                  float* pose, double* pose64, double* fitness, double* inlier_rmse, int* iterations, int* count,
                  int* corr, int* status, void* ws, size_t ws_bytes, void* stream);

/* ---- Point-to-plane ICP for all pairs, with robust kernels ---------------------------------------------------------
 * The loop of Open3D's registration_icp with TransformationEstimationPointToPlane (optionally with a Huber or Tukey
 * kernel) for all nb pairs of a batch in one call.  Arguments, outputs, status, workspace rule, chunked read-back and
 * frozen pairs are spr_icp_pairs'; the additional inputs are
 *   tgt_normals [nt,3] f32   row-aligned with tgt_xyz; used as given, NOT renormalised
 *   kernel                   0 = L2, 1 = Huber, 2 = Tukey (any other value is refused on the host)
 *   kernel_k                 the kernel's parameter k, in the clouds' units; read only when kernel != 0, and then
 *                            refused on the host unless > 0 (NaN is refused)
 * Open3D is not available here and the reference never calls this estimate: the definition below, written from
 * Open3D's published behaviour, is the contract.
 * Contract, per pair, in IEEE float64 on the exactly converted float32 inputs, one rounding per operation, no FMA:
 *   E(T) is EXACTLY that of "ICP for all pairs": the same s', d2, strict threshold and lowest-index tie rule give
 *   corr, count, fitness and inlier_rmse -- the RMSE stays the POINT distance, as in Open3D's RegistrationResult.
 *   For every matched i, with j = corr_i:
 *     a = s'_i, b = tgt_j, n = tgt_normals_j; c = the per-axis minimum of the pair's target cloud (a conditioning
 *     shift: exact, independent of any order)
 *     r  = ((ax-bx) nx + (ay-by) ny) + (az-bz) nz
 *     p  = a - c;  J = [py nz - pz ny, pz nx - px nz, px ny - py nx, nx, ny, nz]        ( = [(a - c) x n ; n] )
 *     w  = 1                                              L2
 *          1 if |r| <= k else k / |r|                     Huber
 *          (1 - (r/k)(r/k))^2 if |r| <= k else 0          Tukey: q = r / k; u = 1 - q q; w = u u
 *     A_kl += (w J_k) J_l for k <= l (21 entries);  g_k += (w J_k) r
 *   A zero normal adds nothing to A and g but counts in fitness and inlier_rmse like any match.
 *   Solve A x = -g by unpivoted LDL^T, A_lk = A_kl.  With m = max_i A_ii, for k = 0 .. 5:
 *     d_k  = A_kk - sum_{p<k} (L_kp d_p) L_kp             subtracted one by one, p ascending
 *     the step is refused unless d_k > 1e-12 m
 *     L_ik = (A_ik - sum_{p<k} (L_ip d_p) L_kp) / d_k     for i = k+1 .. 5, subtracted likewise
 *   y_i = -g_i - sum_{p<i} L_ip y_p (i ascending);  x_i = y_i / d_i - sum_{p>i} L_pi x_p (i descending, p ascending).
 *   U = I when count = 0 or the step is refused (a flat patch has an exact zero pivot: the pose then stays, and the
 *   pair stops after one step because nothing moved).  Deviation: Open3D refuses on |det A| < 1e-6, an absolute
 *   threshold that depends on the clouds' units; the relative pivot rule does not.
 *   Otherwise, with omega = x[0:3], v = x[3:6]:
 *     t = v - omega x c:  t_0 = v_0 - (omega_1 c_2 - omega_2 c_1), t_1 = v_1 - (omega_2 c_0 - omega_0 c_2),
 *                         t_2 = v_2 - (omega_0 c_1 - omega_1 c_0)
 *       (in exact arithmetic (omega, t) is Open3D's minimiser, which linearises about the world origin)
 *     U = [Rz(omega_2) Ry(omega_1) Rx(omega_0) | t], Open3D's TransformVector6dToMatrix4d (not the exponential map);
 *       with s., c. the sine and cosine of omega_0 (x), omega_1 (y), omega_2 (z):
 *       [cz cy, (cz sy) sx - sz cx, (cz sy) cx + sz sx;  sz cy, (sz sy) sx + cz cx, (sz sy) cx - cz sx;  -sy, cy sx, cy cx]
 *   T_0 = pose_init; evaluate E(T_0); then for k = 0 .. max_iter - 1:
 *     T_{k+1} = U o T_k, composed in float64; evaluate E(T_{k+1})
 *     stop after this pass if |fitness_{k+1} - fitness_k| < rel_fitness and |rmse_{k+1} - rmse_k| < rel_rmse
 *   iterations = the number of steps k run; every output is that of the LAST evaluation.
 * One pass over the correspondences serves the evaluation of T_k and the solve for T_{k+1}: a call makes
 * iterations + 1 association passes per pair.  The order of the sums of A, g and d2 is the implementation's, fixed and a
 * function of the pair alone (per-block float64 partials added in block order, no floating-point atomics): every
 * output of a pair has the same bits whatever batch, position or neighbours it is called with, and run to run.  A
 * pair that has stopped is frozen: later passes of the call neither touch it nor do association work for it.
 * Negating every normal of a pair changes no output bit (J and r change sign together).
 * Empty sources and targets are legal (fitness 0, pose = pose_init).  status [nb] i32: 0, or -1 when the pair has a
 * non-finite coordinate, normal or pose: pose = pose_init, fitness = rmse = 0, iterations = count = 0, corr = -1 for
 * that pair only.  The cell-table rule, the read-back rule and the workspace rule are spr_icp_pairs', with
 * spr_icp_plane_pairs_workspace_size(ns, nt, nb).  Out of scope: source-side or symmetric normals, coloured and
 * generalised ICP. */
size_t spr_icp_plane_pairs_workspace_size(int ns, int nt, int nb);
int spr_icp_plane_pairs(const float* src_xyz, const int* src_cu, int ns, const float* tgt_xyz, const float* tgt_normals,
                        const int* tgt_cu, int nt, const double* pose_init, int nb, double max_dist, int max_iter,
                        double rel_fitness, double rel_rmse, int kernel, double kernel_k, float* pose, double* pose64,
                        double* fitness, double* inlier_rmse, int* iterations, int* count, int* corr, int* status,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- Registration metrics for all pairs: RPMNet / DCP errors, modified Chamfer distance, inlier ratio -------------
 * What the reference computes at the end of every experiment (benchmark/benchmark_modelnet.py: compute_metrics, right
 * at batch size 1 only; models/generic_reg_model.py: compute_IR), for all nb pairs of a batch in one call.  Per pair:
 * the source cloud, the reference (target) cloud, optionally the clean raw shape in the reference's frame (Chamfer),
 * optionally a set of correspondences (inlier ratio), the ground-truth pose G and the predicted pose P, src -> tgt.
 * Contract, per pair, in IEEE float64 on the exactly converted float32 inputs, one rounding per operation, no FMA:
 *   dot3     = (a0 b0 + a1 b1) + a2 b2;  T x = dot3(row, x) + t per row;  d2(a, b) as in "ICP for all pairs"
 *   Ginv     = [Rg^T | -(Rg^T tg)];  (A o B)_R[r][q] = dot3(A_R[r][:], B_R[:][q]),  (A o B)_t[r] = dot3(A_R[r][:], B_t) + A_t[r]
 *   C        = Ginv o P;  D = P o Ginv
 *   deg(x)   = (x 180) / pi
 *   e(R)     = (deg(atan2(R21, R22)), deg(-asin(clamp(R20, -1, 1))), deg(atan2(R10, R00)))
 *              -- scipy's as_euler('xyz', degrees=True); at gimbal lock this closed form is the contract
 *   r_mse    = ((u0^2 + u1^2) + u2^2) / 3,  r_mae = ((|u0| + |u1|) + |u2|) / 3    with u = e(Rg) - e(Rp)
 *   t_mse, t_mae: the same with u = tg - tp
 *   err_r_deg = deg(acos(clamp(0.5 (((C00 + C11) + C22) - 1), -1, 1)))
 *   err_t     = sqrt((Ct0^2 + Ct1^2) + Ct2^2);  trans_err = the same of Dt (se3_compare's translation error; its
 *               rotation angle is err_r_deg's in exact arithmetic)
 *   Chamfer (raw_cu != NULL):  a_i = P src_i,  c_j = D raw_j
 *     d2_src_i = min_j d2(a_i, raw_j),  d2_ref_i = min_j d2(ref_i, c_j);  nn_* = the lowest LOCAL j attaining it
 *     chamfer_src = sum_i d2_src_i / n_src,  chamfer_ref = sum_i d2_ref_i / n_ref  (0 for an empty query cloud)
 *     chamfer_dist = chamfer_src + chamfer_ref
 *   Inlier ratio (corr_cu != NULL):
 *     inlier_count = #{k : d2(G corr_src_k, corr_tgt_k) < acceptance_radius * acceptance_radius}   (strict)
 *     inlier_ratio = inlier_count / n_corr                                        (0 for an empty set)
 * d2_* and nn_* are determined exactly by the contract.  The order of the two mean sums is the implementation's, fixed
 * and a function of the pair alone (per-block float64 partials added in block order, no floating-point atomics): every
 * output of a pair has the same bits whatever batch, position or neighbours it is called with, and run to run.
 * metrics [nb, SPR_EVAL_COLS] f64, columns in this order:
 *   r_mse, r_mae, t_mse, t_mae, err_r_deg, err_t, trans_err, chamfer_src, chamfer_ref, chamfer_dist, inlier_count,
 *   inlier_ratio;  a part that was not asked for (raw_cu / corr_cu NULL) leaves its columns 0 and its d2 / nn untouched
 * status [nb] i32: 0;  -1 when the pair has a non-finite coordinate or pose entry: all columns 0, d2 = 0, nn = -1 for
 * that pair only;  -2 when its raw cloud is empty while its source or reference is not: the Chamfer columns 0, d2 = 0,
 * nn = -1, every other column as defined.
 * Nearest neighbours are exact brute force, O(n m) per pair and direction: 8 float64 operations and a compare per
 * (query, target), targets staged in LDS tiles of SPR_EVAL_TILE points, SPR_EVAL_QUERIES queries per workgroup.
 * Right for object-sized clouds (ModelNet: 717 x 2048); a grid-accelerated search for scan-sized clouds is out of scope.
 * The call reads nothing back from the device; a workspace below spr_eval_pairs_workspace_size(ns, nt, nr, nc, nb) is
 * refused before anything is enqueued.
 *   src_xyz [ns,3] f32, src_cu [nb+1] i32; ref_xyz [nt,3], ref_cu; raw_xyz [nr,3], raw_cu (both NULL: no Chamfer);
 *   corr_src, corr_tgt [nc,3] f32, corr_cu [nb+1] (all NULL: no inlier ratio; otherwise acceptance_radius > 0)
 *   pose_gt, pose_pred [nb,3,4] f64
 *   d2_src [ns] f64, nn_src [ns] i32, d2_ref [nt] f64, nn_ref [nt] i32: each may be NULL (not wanted) */
#define SPR_EVAL_COLS 12
#define SPR_EVAL_TILE 256    /* targets per LDS tile */
#define SPR_EVAL_QUERIES 128 /* queries per workgroup */
size_t spr_eval_pairs_workspace_size(int ns, int nt, int nr, int nc, int nb);
int spr_eval_pairs(const float* src_xyz, const int* src_cu, int ns, const float* ref_xyz, const int* ref_cu, int nt,
                   const float* raw_xyz, const int* raw_cu, int nr, const float* corr_src, const float* corr_tgt,
                   const int* corr_cu, int nc, const double* pose_gt, const double* pose_pred, int nb,
                   double acceptance_radius, double* metrics, double* d2_src, int* nn_src, double* d2_ref,
                   int* nn_ref, int* status, void* ws, size_t ws_bytes, void* stream);

/* Per-point input features: spr_kpconv_fwd (impl 0 and 2) runs 2 <= cin <= 8 with any cout >= 1 and at most 16
 * kernel points on the small-Cin kernel (k_kpconv_few: exact f32, the cin = 1 kernel's influence and data movement);
 * spr_kpconv_workspace_bytes covers its support records.  Host only: the dispatch rule, for callers and tests. */
int spr_kpconv_few_supported(int cin, int cout, int n_kp);

/* Encoder stem in inference: the first block's KPConv (cin = 1, x [ns,1]) + per-cloud InstanceNorm + LeakyReLU,
 *   out [nq,cout] = lrelu(IN(spr_kpconv_fwd(...)), slope)
 * without the raw [nq,cout] tensor: only the 16 normalised influence sums per query are kept (in ws) and the rows
 * are formed twice from them, for the statistics and for the output.  Row values have spr_kpconv_fwd's bits; the
 * statistics are summed in float64 over 512-row slices from each cloud's first row (batch invariant) in another order
 * than spr_instnorm's, so a mean or rstd may be the adjacent float32.  cu [nb+1] over the nq rows, max_len_host, eps,
 * out_range / out_range_n as in spr_instnorm; mean_out / rstd_out (or NULL): [nb,cout], receive the statistics.
 * spr_kpconv_stem_supported: cin == 1, cout a multiple of 16, at most 16
 * kernel points; other shapes are refused (the caller uses spr_kpconv_fwd + spr_instnorm). */
int spr_kpconv_stem_supported(int cin, int cout, int n_kp);
size_t spr_kpconv_stem_workspace_size(int nq, int ns, int nb, int max_len_host, int cout);
int spr_kpconv_stem(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int nbr_stride,
                    int kmax, int rows_sorted, const float* x, const float* weights, int cout,
                    const float* kernel_points, int n_kp, float kp_extent, const int* cu, int nb,
                    int max_len_host, float eps, float slope, float* out, float* out_range, int out_range_n,
                    float* mean_out, float* rstd_out, void* ws, size_t ws_bytes, void* stream);

/* ---- a5: per-cloud InstanceNorm (+ residual add) (+ LeakyReLU) ------------
 * Replaces BatchNormBlock.forward (kpconv_blocks.py:497-525: per-cloud
 * nn.InstanceNorm1d, affine=False, eps, biased variance) fused with the
 * LeakyReLU that follows it (kpconv_blocks.py:553-561, :645, :727) and with
 * the residual add of ResnetBottleneckBlock (:741):
 *   out = lrelu(IN(x) + add, slope)      slope = 1 -> no activation
 * x,out [n,c] (may alias); add [n,c] or NULL; cu [nb+1]; max_len_host = an
 * upper bound of the longest cloud (sizes the statistics grid: fixed 512-row
 * slices relative to each cloud, so results are batch-invariant bit for bit).
 * norm = 0 skips the normalisation (out = lrelu(x + add)).
 * out_range (or NULL): out_range_n zeroed slots, a power of two chosen by the caller, that receive partial
 * maxima of |out| (operand-range hand-over, see spr_linear).
 * spr_instnorm_stats: mean / rstd [nb][c] of the statistics passes alone (same workspace).
 */
size_t spr_instnorm_workspace_bytes(int max_len_host, int nb, int c);
int spr_instnorm(const float* x, const int* cu, int n, int nb, int max_len_host, int c,
                 float eps, int norm, const float* add, float slope, float* out,
                 float* out_range, int out_range_n, void* ws, size_t ws_bytes, void* stream);
int spr_instnorm_stats(const float* x, const int* cu, int n, int nb, int max_len_host, int c, float eps,
                       float* mean, float* rstd, void* ws, size_t ws_bytes, void* stream);

/* ---- a5: tail of a ResNet bottleneck block, fused -----------------------------
 * Replaces the last three statements of ResnetBottleneckBlock.forward
 * (kpconv_blocks.py:733-741): unary2 (Linear without bias -> per-cloud
 * InstanceNorm, :556-561), unary_shortcut (the same, or the identity) and
 * leaky_relu(x + shortcut):
 *   out = lrelu(IN(xa wa^T) + (kb > 0 ? IN(xb wb^T) : add), slope)
 * xa [n,ka], wa [n_out,ka]; xb [n,kb], wb [n_out,kb] (kb = 0: xb = wb = NULL and
 * add [n,n_out] or NULL is added instead); cu [nb+1].  The projections are computed
 * twice (statistics pass, output pass) and never written: only `out` goes to memory.
 * Split-fp16 product mode only (spr_set_gemm_mode(1)); ranges as in spr_linear
 * (NULL: measured here); out_range as in spr_instnorm.
 * xa_mean / xa_rstd [nb][ka] (both or neither; NULL = xa is already normalised, xa_slope is then ignored):
 * xa is the RAW input of a per-cloud InstanceNorm + LeakyReLU(xa_slope) (the KPConv output of a bottleneck
 * block, kpconv_blocks.py:717-719 of the reference) whose statistics the caller holds (spr_instnorm_stats);
 * the normalisation runs while a tile is staged -- the normalised tensor is never written.  xa_range is then
 * required and bounds the NORMALISED values: sqrt(longest cloud) is always valid.
 * spr_block_tail_tile_rows: rows per statistics tile of a supported (ka, kb, n_out), 0 if
 * the shape has no kernel (the caller then uses spr_linear + spr_instnorm);
 * spr_block_tail_tiles: the tile table of a batch (int32 [spr_block_tail_tiles_len], 16-byte
 * aligned): the exclusive prefix of ceil(len / tile_rows) per cloud and one {first row, valid
 * rows, cloud} record per tile -- tiles start at each cloud's first row, so a cloud's result
 * never depends on its batch mates.  Depends on cu and tile_rows only: build once per level.
 */
int spr_block_tail_tile_rows(int ka, int kb, int n_out);
size_t spr_block_tail_tiles_len(int n, int nb, int tile_rows);
int spr_block_tail_tiles(const int* cu, int n, int nb, int tile_rows, int* tiles, void* stream);
size_t spr_block_tail_workspace_bytes(int n, int nb, int kb, int n_out, int tile_rows);
int spr_block_tail(const float* xa, int ka, const float* wa, const float* xb, int kb, const float* wb,
                   const float* add, const int* cu, const int* tiles, int n, int nb, int n_out, float eps,
                   float slope, float* out, const float* xa_range, int xa_range_n, const float* wa_range,
                   int wa_range_n, const float* xb_range, int xb_range_n, const float* wb_range,
                   int wb_range_n, float* out_range, int out_range_n, const float* xa_mean,
                   const float* xa_rstd, float xa_slope, void* ws, size_t ws_bytes, void* stream);

/* ---- a5: strided max pooling ----------------------------------------------
 * Replaces max_pool(x, inds) (kpconv_blocks.py:127-143): max over the pooling
 * neighbours, shadow index ns reads a zero row.  idx [nq, idx_stride], first
 * k columns used.
 * order (or NULL = natural order): int32 [nq], a permutation in which the queries are WALKED (spr_cell_order of
 * the query points).  Results are identical; queries in flight together then share support rows, which L2
 * serves instead of HBM (the reference has no counterpart of the order).
 * out_range / out_range_n (or NULL): as in spr_instnorm.
 * spr_cell_order: order [n] = the points of every cloud (cu [nb + 1]) sorted by the Morton code of their cell of
 * size `cell` (clouds in batch order): a spatial walk order for gather operators, not part of any result.
 */
int spr_maxpool_gather(const float* x, int ns, int c, const int* idx, int nq, int idx_stride, int k,
                       const int* order, float* out, float* out_range, int out_range_n, void* stream);
size_t spr_cell_order_workspace_bytes(int n);
int spr_cell_order(const float* xyz, const int* cu, int n, int nb, float cell, int* order, void* ws, size_t ws_bytes,
                   void* stream);

/* ---- dense projection -------------------------------------------------------
 * out[m,n] = act(x[m,k] @ w[n,k]^T + bias[n] + residual[m,n])
 * Replaces the nn.Linear calls on the path: UnaryBlock.mlp
 * (kpconv_blocks.py:549,:557), feat_proj / overlap_predictor
 * (qk_regtr_full.py:47,:85,:176,:248), MultiheadAttention in/out projections
 * and linear1/linear2 (transformer/transformers.py:96-104).
 * bias, residual may be NULL.  k must be a multiple of 32 unless n <= 64.
 * ws: spr_linear_workspace_bytes() bytes of device scratch (the operands'
 * max-|x| partials; may be NULL in mode 0).
 */
size_t spr_linear_workspace_bytes(void);
int spr_linear(const float* x, int m, int k, const float* w, int n, const float* bias,
               const float* residual, int act, float* out, const float* x_range,
               int x_range_n, const float* w_range, int w_range_n, float* out_range,
               int out_range_cap, int* out_range_n_host, void* ws, size_t ws_bytes, void* stream);
/* Operand-range hand-over.  The split-fp16 arithmetic scales every operand tensor by a power of
 * two derived from max |x|; by default spr_linear measures it with a pass over x.  A producer
 * that has just written x can publish the range instead, as an array of per-workgroup partial
 * maxima in device memory (any count; their maximum must bound max |x| from above):
 *   x_range / x_range_n     range of x (NULL: measure);
 *   w_range / w_range_n     range of the weights (NULL: measure).  Weights do not change between
 *     inference calls: measure them once with spr_absmax (spr_range_parts() floats) and pass
 *     the result on every call; with both ranges handed in the call has no pre-pass at all;
 *   out_range (capacity out_range_cap floats; NULL: nothing published): if the GEMM runs with
 *     <= out_range_cap workgroups it writes one partial per workgroup and sets *out_range_n_host
 *     (a HOST int) to their number, else 0 (nothing published).
 * The other operators take and publish ranges under the same argument names: where an operator
 * combines its workgroups' maxima with atomic max (spr_layernorm, spr_instnorm, spr_maxpool_gather,
 * spr_block_tail), the CALLER MUST ZERO the out_range slots beforehand. */
int spr_range_parts(void);
int spr_absmax(const float* x, long rows, int cols, long stride, float* parts, void* stream);
/* max |x| of many contiguous tensors in ONE launch (all weights of a model at the start of a training step).
 * jobs_dev: njobs device records {const float* x; long long n_elements;}; parts_out [njobs][parts_per_job]:
 * row j is a range (parts_per_job partials) of tensor j, usable wherever spr_absmax partials are. */
int spr_absmax_multi(const void* jobs_dev, int njobs, int parts_per_job, float* parts_out, void* stream);

/* Arithmetic of spr_linear (and of the correlation GEMMs inside the matching
 * head):
 *   1 (default) = split-fp16 MFMA: each operand tensor is scaled by a power of
 *     two derived from its measured max |x| (no overflow possible, whatever the
 *     magnitudes), then carried as fp16 hi + fp16 lo; three MFMAs per product,
 *     fp32 accumulation.  Elements within 2^-18 of their tensor's maximum keep 22
 *     significand bits (~2^-22 relative per product); smaller ones keep an
 *     absolute error of 2^-39 max|x|.  ~5x the exact-f32 MFMA rate.
 *   0 = exact f32 MFMA (a k-ordered fmaf chain). */
int spr_set_gemm_mode(int mode);

/* ---- LayerNorm (+ positional embedding add) --------------------------------
 * Replaces norm1/2/3 + with_pos_embed (transformers.py:121,:196-197,:212-214,
 * :234) and the final encoder norm (:46-48).
 *   out_norm = LN(x) (may be NULL); out_pos = LN(x) + pos (NULL if pos NULL)
 *   range_norm / range_pos (each may be NULL): the ranges of the two outputs, published into
 *   spr_layernorm_range_count(m) slots each, which the CALLER MUST ZERO beforehand (the kernel combines its
 *   workgroups' maxima with atomic max; operand-range hand-over, see spr_linear).
 */
int spr_layernorm_range_count(int m);
int spr_layernorm(const float* x, int m, int c, const float* gamma, const float* beta,
                  float eps, const float* pos, float* out_norm, float* out_pos,
                  float* range_norm, float* range_pos, void* stream);

/* ---- a7: sine positional embedding -----------------------------------------
 * Replaces PositionEmbeddingCoordsSine.forward (transformer/
 * position_embedding.py:29-50).  xyz [n,3] -> out [n,d_model].  The distinct frequencies of an axis
 * (d_model / 6) are held in a table of 1024: d_model of 6150 and more is refused.
 */
int spr_posemb_sine(const float* xyz, int n, int d_model, float scale,
                    float temperature, float* out, void* stream);

/* ---- a7: learned positional embedding ----------------------------------------
 * Replaces PositionEmbeddingLearned.forward (transformer/position_embedding.py:53-72; pos_emb_type: learned,
 * qk_regtr_full.py:55-56): the MLP 3 -> 32 -> 64 -> 128 -> 256 -> d_model with a ReLU behind each of the first four
 * layers.  xyz [t,3] -> pe [t,d_model]; d_model must be 256 (anything else is a status error, like spr_xenc_prepare).
 *   params_host: a HOST array of the ten DEVICE pointers mlp.{0,2,4,6,8}.{weight,bias} in that order
 *   (weight [out,in] row-major as nn.Linear keeps it, 16-byte aligned).
 * One fused kernel: a workgroup carries a tile of 64 tokens through all five layers in LDS, the weights stream from
 * L2; no intermediate goes to memory.  Exact f32 arithmetic (layers 2-5 on v_mfma_f32_32x32x2_f32): no operand is
 * scaled, no coordinate or weight magnitude needs a bound, and spr_set_gemm_mode does not change the result.
 * t = 0 returns 0 and writes nothing.
 * spr_posemb_mlp_bwd: the ten parameter gradients (grads_host: HOST array of ten DEVICE pointers, shapes and order of
 *   params_host; fully written, t = 0 writes zeros) of sum(pe * dpe), dpe [t,256] 16-byte aligned.  Nothing is kept
 *   from the forward: one kernel recomputes the activations from xyz, runs the deltas back down
 *   (delta_l = (delta_{l+1} W_{l+1}) relu'(h_l), relu'(0) = 0) and leaves both in ws; the weight gradients are
 *   spr_bgemm products over fixed 256-token records summed by spr_reduce_parts, the bias gradients spr_colsum.
 *   No atomics: two calls on the same inputs give the same bits.  There is no d xyz (coordinates are never
 *   differentiated).  ws: spr_posemb_mlp_bwd_workspace_bytes(t) bytes, 256-byte aligned.
 */
int spr_posemb_mlp(const float* xyz, const float* const* params_host, int t, int d_model, float* pe, void* stream);
size_t spr_posemb_mlp_bwd_workspace_bytes(int t);
int spr_posemb_mlp_bwd(const float* xyz, const float* const* params_host, const float* dpe, int t, int d_model,
                       float* const* grads_host, void* ws, size_t ws_bytes, void* stream);

/* ---- a9: varlen multi-head attention core -----------------------------------
 * Replaces the scaled-dot-product core of the four nn.MultiheadAttention
 * calls per layer (transformers.py:198-227) on packed tokens: segment s
 * attends from its own queries to the keys/values of segment kv_seg[s]
 * (self: kv_seg[s] = s; cross: the partner cloud).  Key padding masks of the
 * reference become segment bounds.
 *   q,k,v: [T, *] f32 with row strides (in floats); head h uses columns
 *   [h*head_dim, (h+1)*head_dim); head_dim must be 32.
 *   cu [nseg+1]; kv_seg [nseg]; out [T, nhead*head_dim] (row stride o_stride)
 *   t = cu[nseg] (total tokens, host copy); max_len_host: upper bound of any
 *   segment length (sizes the grid).  ws: spr_attn_workspace_bytes(t, nseg,
 *   nhead, head_dim) bytes of device scratch (the split-fp16 operand planes;
 *   may be NULL in mode 0).
 *   lse (NULL = not wanted) [t, nhead]: receives log2 sum_j 2^(log2(e) scale q_i.k_j) per query and head for
 *   spr_attn_varlen_bwd (training: what torch's SDPA backward keeps as `logsumexp`).  lse_written (a HOST int,
 *   required only with lse): *lse_written = 0 in exact-f32 mode (attention mode 0, whose core does not
 *   produce it): lse is then untouched.
 */
size_t spr_attn_workspace_bytes(int t, int nseg, int nhead, int head_dim);
int spr_attn_varlen_fwd(const float* q, int q_stride, const float* k, int k_stride, const float* v,
                        int v_stride, const int* cu, const int* kv_seg, int t, int nseg, int max_len_host,
                        int nhead, int head_dim, float scale, float* out, int o_stride, float* lse,
                        int* lse_written, void* ws, size_t ws_bytes, void* stream);

/* In-projection + attention core in one call: replaces
 * F.multi_head_attention_forward's packed in-projection (q, k from x_qk,
 * v from x_v; in_proj_weight [3d, d], in_proj_bias [3d]) followed by the core
 * above -- nn.MultiheadAttention as called at transformers.py:198-227 minus the
 * out-projection.  In split-fp16 mode the projection GEMM writes the attention
 * operand planes straight from its accumulators (no fp32 [t, 3d] round trip);
 * in exact mode it equals spr_linear + spr_attn_varlen_fwd.  d_model = 256.
 *   x_qk, x_v [t, d] contiguous (may be the same pointer); out [t, d].
 *   xqk_range / xv_range (NULL: measured here): the input ranges, as in spr_linear; out_range (or NULL): receives
 *   a bound of the output (1 float: the attention output is a convex combination of value rows), on the fused
 *   split-fp16 path only.
 *   w_prep (or NULL): the weight-side inputs of the fused in-projection -- spr_range_parts() partial
 *   maxima of |w_in| followed by its 3 d row L1 norms -- from spr_attn_inproj_prepare, measured once
 *   per weight version.
 */
size_t spr_attn_inproj_workspace_bytes(int t, int nseg, int nhead, int head_dim);
int spr_attn_inproj_prepare(const float* w_in, int d, float* out, void* stream);
int spr_attn_inproj_varlen_fwd(const float* x_qk, const float* x_v, int t, const float* w_in,
                               const float* b_in, const int* cu, const int* kv_seg, int nseg,
                               int max_len_host, int nhead, int head_dim, float scale,
                               float* out, int o_stride, const float* xqk_range,
                               int xqk_range_n, const float* xv_range, int xv_range_n,
                               float* out_range, const float* w_prep, void* ws, size_t ws_bytes, void* stream);

/* ---- a9, analysis: the attention maps of the varlen core ------------------------------------
 * Replaces the weights nn.MultiheadAttention returns with need_weights=True at the four calls per
 * layer of TransformerCrossEncoderLayer (transformers.py:198-227 pre-norm, :133-165 post-norm), which
 * the reference keeps in satt_weights / xatt_weights (:179-180, :242-243) for get_attentions (:61-82):
 *   P_h[i, j] = softmax_j(scale q_i,h . k_j,h) for the queries of segment s over the keys of segment
 *   kv_seg[s]; per_head = 0 writes the mean over the heads (the reference's default), 1 every head.
 * Own split-fp16 Q / K planes and fp32 row statistics: the result does not depend on spr_set_attn_mode,
 * and two calls on the same inputs are bitwise equal.  Rows sum to 1.
 *   q, k: [t, *] f32 views, row strides q_stride / k_stride (multiples of 4 floats, 16-byte aligned rows),
 *   head h in columns [h*32, (h+1)*32); cu [nseg+1], kv_seg [nseg] as for spr_attn_varlen_fwd;
 *   max_len_host >= every segment length.
 *   place [nseg][5] int64 (device): {element offset into out, row stride, head stride, rows, cols} of
 *   segment s.  Its rows x cols entries (per head) are ALL written: the Lq x Lk block of probabilities in
 *   the top-left corner, exact zeros elsewhere (padded query rows and key columns), nothing outside.
 *   rows / cols <= max_rows_host / max_cols_host (they size the grid).  This fills the reference's
 *   padded (B, Ls, Ls), (B, Ls, Lt) and (B, H, L, S) tensors in place in one call.
 *   ws: spr_attn_probs_workspace_bytes(t, nhead, head_dim) bytes (0 for bad sizes).  head_dim must be 32.
 */
size_t spr_attn_probs_workspace_bytes(int t, int nhead, int head_dim);
int spr_attn_probs(const float* q, int q_stride, const float* k, int k_stride, const int* cu,
                   const int* kv_seg, int t, int nseg, int max_len_host, int nhead, int head_dim,
                   float scale, int per_head, float* out, const long long* place, int max_rows_host,
                   int max_cols_host, void* ws, size_t ws_bytes, void* stream);

/* ---- a9, fused: the whole cross-encoder stack of an inference forward -----------------------
 * Replaces TransformerCrossEncoder.forward (models/transformer/transformers.py:45-80) over
 * TransformerCrossEncoderLayer.forward_pre (:184-245) for the configuration every shipped experiment
 * uses (pre_norm, sa_val_has_pos_emb, ca_val_has_pos_emb, ReLU, dropout 0, d_model 256 = 8 x 32):
 * per layer two attention cores and two fused row chains (csrc/xenc.hip) -- out-projection +
 * residual, LayerNorm (+ positional embedding), feed-forward block, next in-projection -- that keep
 * every intermediate on the chip and write the attention operand planes directly.
 * spr_xenc_prepare: once per weight version.  layer_ptrs_host = SPR_XENC_PTRS_PER_LAYER device
 *   pointers per layer in the order self_attn.{in_proj_weight, in_proj_bias, out_proj.weight,
 *   out_proj.bias}, multihead_attn.{same four}, linear1.{weight, bias}, linear2.{weight, bias},
 *   norm1.{weight, bias}, norm2.{..}, norm3.{..}; eps_host = 3 floats per layer (norm1..3);
 *   final_g / final_b = the stack's final LayerNorm or NULL; pos_bound = max |pos| (1 for the sine
 *   embedding).  Lays the weights out as split-fp16 MFMA fragments in `prepared`
 *   (spr_xenc_prepared_bytes, device) and fills the host-side plan (spr_xenc_plan_bytes, opaque).
 *   Synchronises the stream (one device->host read of the parameter statistics).  The plan refers to
 *   `prepared` and to the bias / LayerNorm parameters themselves: keep all of them alive and unchanged.
 * spr_xenc_forward: x, pos, out [t, 256]; cu [nseg + 1]; kv_self / kv_cross [nseg] = key segment of
 *   every query segment.  Split-fp16 arithmetic only (gemm mode 1, attention mode 1 or 2).
 */
#define SPR_XENC_PTRS_PER_LAYER 18
size_t spr_xenc_prepared_bytes(int n_layers, int d_ff);
size_t spr_xenc_plan_bytes(void);
int spr_xenc_prepare(const void* const* layer_ptrs_host, const float* eps_host, int n_layers,
                     int d_model, int nhead, int d_ff, const float* final_g, const float* final_b,
                     float final_eps, float pos_bound, void* prepared, size_t prepared_bytes,
                     void* plan_host, size_t plan_bytes, void* stream);
size_t spr_xenc_workspace_bytes(int t, int nseg);
int spr_xenc_forward(const void* plan_host, const float* x, const float* pos, const int* cu,
                     const int* kv_self, const int* kv_cross, int t, int nseg, int max_len_host,
                     float* out, void* ws, size_t ws_bytes, void* stream);

/* Backward of spr_attn_varlen_fwd (the graph torch autograd builds for the attention core of
 * nn.MultiheadAttention, transformers.py:198-227), flash style: the Lq x Lk matrices are recomputed
 * tile by tile and never written.  out = the forward's output, dout = its gradient; kv_seg must be a
 * permutation of the segments, q_seg its inverse.  Exact f32 MFMA, fixed summation order (bitwise
 * reproducible).  dq, dk, dv [t, nhead * 32] contiguous, fully written.  head_dim = 32.
 * lse: what spr_attn_varlen_fwd handed out for the same q, k (the backward then skips its own pass over the
 * keys); NULL = computed here.
 * ws: spr_attn_bwd_workspace_bytes has room for the pre-split operand planes of the split-fp16 form (faster);
 * with at least spr_attn_bwd_min_workspace_bytes the kernels convert the fp32 tiles they stage themselves.
 * t rounded up to whole 64-row tiles + 64 * nseg must stay below 2^31 (the padded plane width is an int).
 */
size_t spr_attn_bwd_workspace_bytes(int t, int nseg, int nhead);
size_t spr_attn_bwd_min_workspace_bytes(int t, int nhead);
int spr_attn_varlen_bwd(const float* q, int q_stride, const float* k, int k_stride, const float* v,
                        int v_stride, const float* out, int o_stride, const float* dout, int do_stride,
                        const float* lse, const int* cu, const int* kv_seg, const int* q_seg, int t, int nseg,
                        int max_len_host, int nhead, int head_dim, float scale, float* dq, float* dk,
                        float* dv, void* ws, size_t ws_bytes, void* stream);

/* Arithmetic of the attention core:
 *   1 = split-fp16 MFMA (Q, K, V and the probabilities carried as fp16
 *     hi + lo; Q/K balanced and V scaled by powers of two derived from measured
 *     or derived bounds, so no magnitude overflows fp16; fp32 accumulation and
 *     softmax; fp32-level accuracy);
 *   0 = exact f32 MFMA;
 *   2 = single-pass fp16 MFMA (hi planes only: 11-bit operands, fp32 softmax and
 *     accumulators; 1/3 of the matrix-core work -- the throughput mode BASELINE
 *     configs[4] names; ~1e-3 relative on the attention output);
 *   3 = split-fp16 scores, the probabilities as ONE fp16 plane (rounded toward
 *     zero) whose rounded values also form the row sum: exact convex combination
 *     of the value rows with weights perturbed by < 2^-10 each (5e-6 of the
 *     output scale on flat rows of ~2 000 keys, up to ~3e-4 on rows carried by a
 *     few keys); 20 instead of 24 MFMAs per 64-key tile;
 *   4 (default) = as 1, the lo plane of the probabilities only on
 *     the 32-key blocks that hold a weight of at least 2^-5 of the running row
 *     sum: every key that carries a row is exact as in mode 1, the many small
 *     weights travel in one fp16 plane rounded to nearest (their rounded values
 *     also form the row sum).  Error of the small weights: 2^-12 / sqrt(3 n) of
 *     the value spread for n comparable keys -- <= 3e-5 of the output scale on
 *     every tested distribution, 3e-6 on the bench's rows of ~2 000 keys (mode
 *     1: 1e-6), and equal to mode 1 on peaked rows (DESIGN.md section 4,
 *     profiles/r05_attn_mode_accuracy.txt).  22-23 instead of 24 MFMAs per
 *     64-key tile and a third fewer conversion instructions. */
int spr_set_attn_mode(int mode);

/* ---- a11: dual-softmax matching ---------------------------------------------
 * Replaces the correlation / dual softmax / arg-max block of
 * RegTR.softmax_correlation (qk_regtr_full.py:453-479, :565-588) for all pairs
 * at once.  Pair b: src tokens = segment b, tgt tokens = segment b + npairs.
 *   feat [T, d]; cu [2*npairs+1]
 *   If N_b > M_b : one match per tgt token  (val,ind over src, len M_b)
 *   else         : one match per src token  (val,ind over tgt, len N_b)
 *   match_val / match_ind are written at the packed position of the token
 *   that owns the match (tgt token when N>M, else src token); ind is LOCAL to
 *   the partner cloud.  corr_ws: caller scratch for the correlation matrices,
 *   size from spr_match_workspace_bytes (host needs the seg lengths).
 *   match_val2 (may be NULL): the runner-up value of every match -- what RegTR.ratio_test needs
 *   (Lowe ratio, qk_regtr_full.py:370-384; cfg.use_ratio_test).
 */
size_t spr_match_workspace_bytes(const int* cu_host, int npairs);
int spr_match_dualsoftmax(const float* feat, int d, const int* cu,
                          const int* cu_host, int npairs, float* match_val,
                          float* match_val2, int* match_ind, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- pose-hypothesis residuals (config-off refinements) -------
 * spr_pose_residuals: res[i] = || b_i - T_s a_i || with one pose per set s of pair_cu
 *   (RegTR.recompute_weights / local_global_registration, qk_regtr_full.py:386-398);
 *   total_host = pair_cu[npairs] (host copy, sizes the grid).
 * spr_pose_scores: score[h] = mean_i || b_i - T_h a_i || for nh hypotheses over ONE point
 *   set (the RANSAC loop of qk_regtr_full.py:400-421, all hypotheses in one launch).
 */
int spr_pose_residuals(const float* pose, const float* a, const float* b, const int* pair_cu,
                       int npairs, int total_host, float* res, void* stream);
int spr_pose_scores(const float* poses, int nh, const float* a, const float* b, int n,
                    float* score, void* stream);

/* ---- a12: weighted Procrustes / Kabsch --------------------------------------
 * Replaces compute_rigid_transform(a, b, weights) (utils/se3_torch.py:109-163)
 * batched over pairs; 3x3 SVD by one-sided Jacobi in registers.
 *   a,b [T,3] packed by pair_cu [npairs+1]; w [T]; out [npairs,3,4].
 */
int spr_weighted_procrustes(const float* a, const float* b, const float* w,
                            const int* pair_cu, int npairs, float* out_pose,
                            void* stream);

/* ---- the config-off refinements for all pairs in one call -------------------
 * Replaces the per-pair tail of RegTR.softmax_correlation (qk_regtr_full.py:370-398 ratio_test / recompute_weights /
 * local_global_registration, :465-553 and :573-658): one launch, one workgroup per pair.
 * Inputs: val / val2 / ind [t_total] as spr_match_dualsoftmax writes them (val2 may be NULL without
 * SPR_REFINE_RATIO), overlap [t_total] f32, xyz [t_total,3] f32, cu [2*npairs+1] i32 (cu[2*npairs] = t_total);
 * k_b [npairs] i32 entries kept per pair and out_cu [npairs+1] i32 their exclusive prefix (device; the caller
 * computes both on the host and uploads them in one copy; out_cu[b+1] - out_cu[b] = k_b[b] <= n_b).
 * Per pair, N / M the src / tgt counts, in this order:
 *   1. the "own" side carries the matches: the tgt tokens when N > M, else the src tokens; n = min(N, M) entries
 *   2. RATIO:    v = (val2 / v < lowe_thres) ? v : 0     correctly rounded f32 divide; 0/0 fails the test
 *   3. MEDIAN:   v = (v > med) ? v : 0,  med = the element at sorted (ascending) position (n-1)/2, exact
 *   4. OVERLAP:  ov = overlap_src * overlap_tgt of (entry, partner ind);  v *= ov unless OVERLAP_W
 *   5. TOPK:     the k_b largest v in descending order, ties to the lower position; without TOPK k_b = n and the
 *                order is the token order
 *      outputs in that order at out_cu[b]: val_out f32, src_pts / tgt_pts [.,3] f32 (the entry's own point and its
 *      partner's; SINKHORN: the src and the tgt point at the entry's position, no partner gather), ind_out i64 =
 *      the partner index, or with TOPK the entry's position (what the reference's ind_list holds after its topk)
 *   6. pose = the solve of spr_weighted_procrustes on the output points, weights ov (OVERLAP_W) else v; with
 *      pose_in [npairs,3,4] (required by SINKHORN) no solve: pose = pose_in
 *   7. LGR: n_steps x { res = ||b - (R a + t)|| in spr_pose_residuals' arithmetic; w *= (res < acceptance_radius)
 *      (w starts as v); pose = solve(w) }
 * pose [npairs,3,4].  A pair's outputs depend on that pair's inputs only: fixed reduction order, no atomics -- the
 * same bits alone or at any place in any batch.
 * status [npairs] i32 (device, no host read here): 0; SPR_REFINE_BAD_INDEX when an ind of the own side lies outside
 * the partner cloud (the entry is then treated as matched to partner 0: never a wild read); SPR_REFINE_BAD_LAYOUT
 * when cu / k_b / out_cu contradict each other or n_b > max_n (pose zeros, nothing else written).
 * max_n: the largest n_b (host).  Up to 4 096 entries a pair's working set (20 bytes per entry) stays in LDS; above,
 * it lives in `ws` (spr_refine_pairs_workspace_bytes, 0 when max_n <= 4 096); max_n > SPR_REFINE_MAX_N is refused
 * with a status return.  OVERLAP_W needs OVERLAP, RATIO needs val2, SINKHORN needs pose_in (status return).
 */
#define SPR_REFINE_RATIO 1
#define SPR_REFINE_MEDIAN 2
#define SPR_REFINE_OVERLAP 4
#define SPR_REFINE_OVERLAP_W 8
#define SPR_REFINE_TOPK 16
#define SPR_REFINE_LGR 32
#define SPR_REFINE_SINKHORN 64
#define SPR_REFINE_ALL_FLAGS 127
#define SPR_REFINE_MAX_N 16384
#define SPR_REFINE_BAD_INDEX 1
#define SPR_REFINE_BAD_LAYOUT 2
size_t spr_refine_pairs_workspace_bytes(int npairs, int max_n);
int spr_refine_pairs(const float* val, const float* val2, const int* ind, const float* overlap, const float* xyz,
                     const int* cu, int npairs, int t_total, const int* k_b, const int* out_cu, int flags,
                     float lowe_thres, float acceptance_radius, int n_steps, const float* pose_in, int max_n,
                     float* pose, float* val_out, long long* ind_out, float* src_pts, float* tgt_pts, int* status,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- RANSAC for all pairs in one call (cfg.use_ransac) ------------------------
 * Replaces the per-pair loop of RegTR.ransac (qk_regtr_full.py:400-421): per pair n_hyp random `sample`-point subsets
 * WITH replacement, compute_rigid_transform on each, the hypothesis with the lowest mean residual over all of the
 * pair's correspondences wins.  Two launches for the whole batch; no workspace (score and hyp_pose are outputs).
 * a, b [T,3] f32 and w [T] f32 packed by set_cu [npairs+1] i32 (device) -- exactly what spr_refine_pairs returns as
 * src_pts, tgt_pts, val_out and out_cu; pair p has n_p = set_cu[p+1] - set_cu[p] entries.
 *
 * 1. Draws (idx == NULL).  Philox4x32-10 with the key and counter layout of the augmentation draw contract above,
 *    stream tag 3, side 0.  With SB = (sample + 3) / 4, sample s of hypothesis h of a pair with key k (< 2^63) and n
 *    entries is word s & 3 of the block with
 *      counter = (h * SB + (s >> 2), q & 0xffffffff, 3, q >> 32),  q = 2 k,   key = (seed & 0xffffffff, seed >> 32)
 *      idx = (uint64(word) * n) >> 32
 *    Multiply-shift without rejection: an index is over-represented by at most n / 2^32 (relative 3e-6 at n = 16 384).
 *    A pair's draws depend on (seed, pair_key, n, n_hyp, sample) only.  Calls with n_hyp * SB >= 2^32 are refused with
 *    a status return.  spr_ransac_draw is the same function on the host (the known-answer entry; n_host [npairs]).
 *    With idx [npairs, n_hyp, sample] i32 (device) the samples are read instead and seed / pair_key are unused.
 * 2. Hypothesis h = compute_rigid_transform (utils/se3_torch.py:109-163) on the `sample` gathered triples
 *    (a[i], b[i], w[i]); duplicates count as often as they are drawn.  Float64 throughout, the arithmetic of
 *    spr_weighted_procrustes: w~ = w / max(sum w, 1e-6), centroids, covariance sum (a - abar)(b - bbar)^T w~, one-sided
 *    Jacobi SVD, the det <= 0 flip, t = bbar - R abar; the result is rounded to float32 into hyp_pose.  Summation
 *    order, for the seven first-pass sums and the nine covariance entries alike: lane l of the hypothesis's wave adds
 *    its samples l, l + 64, l + 128, ... in ascending order; the 64 lane sums are then combined by the butterfly
 *    x += x(lane ^ 32), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  The order does not depend on what else is in the batch.
 * 3. score[h] = mean_i || b_i - (R a_i + t) || over all n entries from the ROUNDED float32 pose, in spr_pose_scores'
 *    float32 arithmetic and order: v_r = b_r - (((x R_r0 + y R_r1) + z R_r2) + t_r), d2 = (v_0^2 + v_1^2) + v_2^2,
 *    lane l adds sqrtf(d2) of entries l, l + 64, ... ascending, the same butterfly, then / (float)n.  So score[p] is
 *    bit-equal to spr_pose_scores(hyp_pose[p], a_p, b_p) (a NaN is a NaN in both; its sign and payload are not
 *    specified).
 * 4. best = 0; for h = 1 .. n_hyp-1: if (score[h] < score[best]) best = h.  The first minimum; a NaN never wins; if
 *    score[0] is NaN, best stays 0.  pose[p] is a bit copy of hyp_pose[p][best].
 * 5. A pair's outputs depend on that pair's inputs and key only: no atomics, the same bits alone or at any place in
 *    any batch.  status [npairs] i32 stays on the device (nothing here reads it back): 0 or
 *      SPR_RANSAC_EMPTY       n_p == 0: pose = [I | 0], best = -1, score / hyp_pose of the pair not written
 *      SPR_RANSAC_BAD_INDEX   an explicit idx outside [0, n_p): that sample is taken as 0, never a wild read
 *      SPR_RANSAC_BAD_LAYOUT  set_cu does not ascend from 0 (anywhere: every pair then reports it): pose zeros, nothing
 *                             else written.  set_cu[npairs] <= T is the caller's to guarantee.
 * pose [npairs,3,4] f32, best [npairs] i32, score [npairs,n_hyp] f32, hyp_pose [npairs,n_hyp,3,4] f32.
 * At most 65 535 pairs per call.
 */
#define SPR_RANSAC_EMPTY 1
#define SPR_RANSAC_BAD_INDEX 2
#define SPR_RANSAC_BAD_LAYOUT 4
int spr_ransac_draw(uint64_t seed, const uint64_t* pair_key_host, const int* n_host, int npairs, int n_hyp,
                    int sample, int* idx_host);
int spr_ransac_pairs(const float* a, const float* b, const float* w, const int* set_cu, int npairs, int n_hyp,
                     int sample, uint64_t seed, const uint64_t* pair_key, const int* idx, float* pose, int* best,
                     float* score, float* hyp_pose, int* status, void* stream);

/* ---- a13: Sinkhorn (slack) soft correspondences -----------------------------
 * Replaces the Sinkhorn branch of softmax_correlation
 * (qk_regtr_full.py:525-536 / :635-647) + sinkhorn() and the weighted target
 * of compute_rigid_transform_with_sinkhorn (utils/se3_torch.py:166-239):
 *   score = clamp(F_s F_t^T / sqrt(d), min 0)
 *   affinity = -(score - softplus(alpha)) / (exp(beta) + 0.02)
 *   n_iters x (row normalise incl. slack col; col normalise incl. slack row)
 *   P = exp(.), w_i = sum_j P_ij, t_hat_i = sum_j P_ij tgt_j / (w_i + 1e-6)
 * alpha, beta: DEVICE pointers to the model's learnable scalars
 * (qk_regtr_full.py:77-78) -- read by the kernel, no host round trip.
 * Outputs per src token: w [Tsrc], t_hat [Tsrc,3] (packed like the src
 * segments).  Feed (src_xyz, t_hat, w) to spr_weighted_procrustes.
 * The scratch holds the scaled correlation (the same matrices as
 * spr_match_dualsoftmax); the affinity is evaluated as the passes read it.
 */
size_t spr_sinkhorn_workspace_bytes(const int* cu_host, int npairs);
int spr_sinkhorn_correspondences(const float* feat, int d, const float* xyz,
                                 const int* cu, const int* cu_host, int npairs,
                                 const float* alpha, const float* beta, int n_iters,
                                 int slack, float* out_w, float* out_that,
                                 void* ws, size_t ws_bytes, void* stream);

/* spr_match_dualsoftmax + spr_sinkhorn_correspondences of the same features in one call -- RegTR's inference
 * forward runs them back to back on the conditioned features (qk_regtr_full.py:453-479 then :525-536).  The scaled
 * correlation matrices are computed and stored once; the Sinkhorn passes evaluate the affinity as they read them.
 * Outputs bit for bit those of the two separate calls; match_val2 may be NULL; workspace:
 * spr_match_workspace_bytes. */
int spr_match_sinkhorn(const float* feat, int d, const float* xyz, const int* cu, const int* cu_host,
                       int npairs, const float* alpha, const float* beta, int n_iters, float* match_val,
                       float* match_val2, int* match_ind, float* out_w, float* out_that, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- small helpers ----------------------------------------------------------*/
/* out[i] = x[idx[i]] rows of width c (idx i32, rows >= n_src read zeros). */
int spr_gather_rows(const float* x, int n_src, int c, const int* idx, int n,
                    float* out, void* stream);

/* ---- decoder: nearest upsample + skip concatenation + unary projection in one GEMM ----------
 * Replaces NearestUpsampleBlock.forward -> closest_pool (kpconv_blocks.py:757-768, :112-124), the torch.cat of
 * KPFDecoder.forward (kpconv.py:156-158) and the UnaryBlock.mlp behind it (kpconv_blocks.py:549,:557):
 *   y[i, :] = [ xc[idx0[i], :] | xs[i, :] ] . w^T        (no bias, no activation, no norm)
 * xc [nc, kc] coarse features, xs [n, ks] skip features, w [n_out, kc + ks] = UnaryBlock.mlp.weight, y [n, n_out],
 * all f32 row-major.  idx0[i] = idx[i * idx_stride]: column 0 of an i32 [n, idx_stride] matrix (idx_stride >= 1), so
 * the int32 upsamples matrix of the pyramid goes in as it is.  A row whose index is >= nc (the shadow index) or < 0
 * contributes a zero coarse row (closest_pool's appended zero row, spr_gather_rows' rule); the call never reads
 * outside xc.  The gathered and the concatenated rows are never written: the tiles gather while they are staged.
 * nc >= 1; n = 0 is legal (nothing is launched).  kc and ks multiples of 32, n_out >= 32 (status 2 otherwise).
 * Arithmetic follows spr_set_gemm_mode.  Mode 1: xc and xs share ONE power-of-two scale, taken from the larger of
 *   their two ranges, so the result has the error bound of spr_linear on the concatenated tensor; mode 0: exact f32,
 *   one fmaf chain over the kc + ks columns.  The reduction order is fixed and there are no atomics: a row's bits
 *   depend on that row's operands (and, in mode 1, on the two scales) only -- not on its position or on the batch.
 * xc_range / xs_range / w_range (+ counts): operand ranges as in spr_linear (NULL = measured here; a range of xc
 *   bounds all of its rows, gathered or not).  out_range / out_range_cap / out_range_n_host: published like
 *   spr_linear's without residual (one partial per workgroup in mode 1 when they fit, else *out_range_n_host = 0).
 * ws: spr_upsample_unary_workspace_size() bytes of device scratch (the three ranges' partials; unused in mode 0).
 * spr_upsample_unary_supported: 1 where the fused call is the host layer's default for the shape, 0 where it takes
 *   gather + two spr_linear calls instead (no kernel for the shape, or none that measured faster).
 */
int spr_upsample_unary_supported(int kc, int ks, int n_out);
size_t spr_upsample_unary_workspace_size(void);
int spr_upsample_unary(const float* xc, int nc, int kc, const float* xs, int n, int ks, const int* idx,
                       int idx_stride, const float* w, int n_out, float* y, const float* xc_range, int xc_range_n,
                       const float* xs_range, int xs_range_n, const float* w_range, int w_range_n,
                       float* out_range, int out_range_cap, int* out_range_n_host, void* ws, size_t ws_bytes,
                       void* stream);

/* ---- pair assembly: encoded clouds -> the token layout of a list of pairs ---------
 * RegTR.register (regtr.py): a cloud is encoded once (pyramid, KPConv encoder, feat_proj) and used by
 * any number of pairs.  x [t_in, c] holds the packed rows of n_clouds clouds (cu [n_clouds + 1]);
 * y [t_out, c] receives 2 * npairs segments stacked [src_0..src_{P-1}, tgt_0..tgt_{P-1}]: segment s is a
 * copy of cloud src_idx[s] for s < npairs and of cloud tgt_idx[s - npairs] otherwise.  cu_out
 * [2 * npairs + 1] is the exclusive prefix of the output segment lengths, built by the caller from the
 * host-side cloud lengths (t_out = cu_out[2 * npairs]); src_idx / tgt_idx [npairs] i32.  One launch,
 * whatever the number of pairs; 16-byte accesses when c % 4 == 0 and x, y are 16-byte aligned (tokens),
 * 4-byte accesses otherwise (c = 3: the superpoint coordinates).  Rows whose source would lie outside
 * the indexed cloud (an index outside [0, n_clouds), a cu_out that does not match the clouds) are zeros.
 */
int spr_pair_gather(const float* x, int t_in, int c, const int* cu, int n_clouds,
                    const int* src_idx, const int* tgt_idx, int npairs, const int* cu_out,
                    int t_out, float* y, void* stream);

/* ---- training over shared clouds: the pair assembly's backward and the labels in pair layout ------
 * RegTR.forward on a batch of clouds and pairs (shared_clouds.py): a cloud is encoded once per step,
 * with gradients, and used by any number of the step's pairs.
 *
 * spr_pair_gather_bwd: gx [t_in, c] from gy [t_out, c], the backward of spr_pair_gather (same cu
 *   [n_clouds + 1], cu_out [2 * npairs + 1], t_in, t_out, c).  The segments that copied a cloud come as
 *   a use list in CSR form: use_seg[use_ptr[k] .. use_ptr[k + 1]) are the output segments (0 ..
 *   2 * npairs - 1) that are copies of cloud k, in ascending order; use_ptr [n_clouds + 1], use_seg
 *   [2 * npairs], both built on the host.  Row i of cloud k (input row cu[k] + i) is the sum over k's
 *   uses s, in the stored order, of gy row cu_out[s] + i, accumulated in registers and stored once: a
 *   fixed order whatever the launch geometry, no atomics.  EVERY row of gx is written (the caller
 *   clears nothing): rows of a cloud without uses, and rows behind cu[n_clouds], are zeros.  A use whose
 *   segment is shorter than its cloud contributes zeros for the rows it lacks, a segment index outside
 *   [0, 2 * npairs) contributes nothing, use_ptr entries are clamped to [0, 2 * npairs]: zeros, never
 *   foreign memory.  16-byte accesses when c % 4 == 0 and gy, gx are 16-byte aligned, 4-byte otherwise.
 *
 * spr_overlap_pool_pairs: one level of compute_overlaps (spr_overlap_pool below; backbone_kpconv/
 *   kpconv.py:552-578) for labels in PAIR layout over a pool matrix in CLOUD layout.  ov_prev [n_prev]:
 *   the previous level's values, segment after segment (cu_out_prev [2 * npairs + 1]); pool
 *   [n_pool_rows, w] with row stride pool_stride: the encode call's pool matrix of this level, whose
 *   entries index the previous level's rows of all clouds (cu_prev [n_clouds + 1]) and whose rows are
 *   this level's rows of all clouds (cu_cur [n_clouds + 1]); seg_cloud [2 * npairs]: the cloud each
 *   segment copies; out [nq], segment after segment (cu_out_cur [2 * npairs + 1]).  Output row r of
 *   segment s, a copy of cloud k, reads pool row cu_cur[k] + (r - cu_out_cur[s]); an entry id counts
 *   when cu_prev[k] <= id < cu_prev[k + 1] and then reads ov_prev[cu_out_prev[s] + id - cu_prev[k]].
 *   out[r] = clamp(sum / count, 0, 1) with the columns in ascending order and 0 / 0 = NaN: the
 *   arithmetic of spr_overlap_pool, bit for bit.  Nothing outside the segment's own labels is read: a
 *   cloud index outside [0, n_clouds), a pool row outside the cloud's, a label outside the segment's
 *   (or outside ov_prev) does not count, and a row left without a counted entry is NaN like a row of
 *   shadow entries.  No workspace.
 */
int spr_pair_gather_bwd(const float* gy, int t_out, int c, const int* cu, int n_clouds,
                        const int* use_ptr, const int* use_seg, int npairs, const int* cu_out,
                        int t_in, float* gx, void* stream);
int spr_overlap_pool_pairs(const float* ov_prev, int n_prev, const int* pool, int pool_stride, int w,
                           int n_pool_rows, const int* cu_prev, const int* cu_cur, int n_clouds,
                           const int* seg_cloud, int npairs, const int* cu_out_prev,
                           const int* cu_out_cur, int nq, float* out, void* stream);

/* ---- losses (forward) of RegTR.compute_loss -- SURVEY 8f row 1 --------------
 * models/qk_regtr_full.py:313-368.  Deterministic reductions (fixed partition,
 * float64 accumulation).  Scalars are written to device memory (out[0]).
 *
 * spr_overlap_pool: one level of compute_overlaps (backbone_kpconv/kpconv.py:
 *   552-578): out[q] = clamp(mean over the valid pool entries of ov_prev, 0, 1).
 * spr_bce_logits_mean: nn.BCEWithLogitsLoss(reduction='mean') (:90, :329).
 * spr_infonce_pair: InfoNCELossFull.compute_infonce (models/losses/
 *   feature_loss.py:268-296) for ONE pair; anchor_xyz are the source keypoints,
 *   transformed by pose_gt [3,4] inside (se3_transform, :341-345).
 * spr_transform_l1_pair: mean |T_gt x - T_pred x| over one pair's keypoints
 *   (:349-355).   spr_sum_scaled: out[0] = scale * sum(values[0..n)).
 * ws: spr_loss_workspace_bytes(max anchors, max positives, d) covers all four.  spr_infonce_pair and its backward
 *   accept d <= 46 336 (d * d is an int in their launches; the query cannot wrap size_t inside that range).
 */
size_t spr_loss_workspace_bytes(int n_max, int m_max, int d);
int spr_overlap_pool(const float* ov_prev, int ns_prev, const int* pool,
                     int pool_stride, int w, int nq, float* out, void* stream);
int spr_bce_logits_mean(const float* x, const float* y, int n, float* out,
                        void* ws, size_t ws_bytes, void* stream);
int spr_infonce_pair(const float* anchor_feat, int n, const float* positive_feat,
                     int m, int d, const float* anchor_xyz, const float* pose_gt,
                     const float* positive_xyz, const float* W, float r_p,
                     float r_n, float* out, void* ws, size_t ws_bytes,
                     void* stream);
int spr_transform_l1_pair(const float* pose_gt, const float* pose_pred,
                          const float* xyz, int n, float* out, void* ws,
                          size_t ws_bytes, void* stream);
int spr_sum_scaled(const float* values, int n, float scale, float* out,
                   void* stream);

/* ==== backward ===============================================
 * The reference trains through the path with torch autograd
 * (models/generic_reg_model.py:82-84 training_step -> trainer.py:107-124
 * backward / clip / step).  These entry points are the explicit gradients of the
 * operators above; autograd.py wires them into torch.autograd.Function objects.
 *
 * spr_bgemm: batched strided exact-f32 GEMM, the matrix-product workhorse
 *   C_b(i,j) = alpha * sum_k A_b(i,k) B_b(k,j) + beta * C_b(i,j),
 *   X_b(p,q) = X[x_off_b + p * sx_p + q * sx_q]; desc: device array of nbatch records
 *   {int64 a_off, b_off, c_off; int32 m, n, k, pad} (element offsets / sizes per batch).
 *   Gives dX = dY W, dW = dY^T X (nn.Linear), the KPConv weight / feature gradients
 *   and every product of the attention backward.
 * spr_reduce_parts: out[j] (+)= scale * sum_p parts[p][j] in fixed order (deterministic split-K).
 * spr_act_bwd: dy * act'(y) for SPR_ACT_RELU / SPR_ACT_SIGMOID.   spr_colsum: bias gradients.
 * spr_layernorm_bwd / spr_instnorm_bwd / spr_maxpool_bwd / spr_scatter_rows_add: gradients of
 *   spr_layernorm (both outputs), spr_instnorm (incl. fused add + LeakyReLU), spr_maxpool_gather,
 *   spr_gather_rows.
 * spr_kpconv_weighted_features: recomputes wf[n,p,c] = sum_k infl[n,p,k] x[idx[n,k],c]
 *   (kpconv_blocks.py:394) and the neighbour count (:409-411) from the per-support flags the
 *   forward computes (same kernel, same summation order; ws: spr_kpconv_weighted_features_workspace_bytes(ns)).
 *   spr_kpconv_bwd_dx scatters d wf back to d x; dwf_range: the max |dwf| partials published by the product
 *   that wrote dwf (spr_linear out_range); NULL = measured.  Together with two spr_bgemm calls = KPConv backward.
 * spr_softmax_rows / spr_softmax_bwd_rows: row softmax of per-batch matrices (located by
 *   c_off, m rows, n columns of the same descriptor records) and its backward -- the
 *   non-GEMM steps of the attention backward.
 */
int spr_bgemm(const float* A, const float* B, float* C, const void* desc_dev, int nbatch,
              int max_m, int max_n, long sa_i, long sa_k, long sb_k, long sb_j, long sc_i,
              long sc_j, float alpha, float beta, void* stream);
/* out[nl, nr] = L[rows, nl]^T R[rows, nr] (row-major, contiguous) with float64 accumulation and a
 * fixed-order reduction: weight gradients that are long, nearly cancelling sums (the first KPConv's
 * dW = wf^T g over every point of the batch, kpconv_blocks.py:401-406 differentiated).  nl * nr <= 65536. */
/* dW = dY^T X in the forward's arithmetic (range-scaled split-fp16 MFMA, fp32 accumulation): per-batch partial
 * products parts[b][nl][nr] over `chunk` rows each, summed by spr_reduce_parts (fixed order).  L [rows, nl],
 * R [rows, nr] row-major; nl, nr multiples of 4, chunk a multiple of 16; ranges as in spr_linear. */
size_t spr_tn_product_split_workspace_bytes(void);
int spr_tn_product_split(const float* L, const float* R, long rows, int nl, int nr, int chunk,
                         const float* l_range, int l_range_n, const float* r_range, int r_range_n,
                         float* parts, void* ws, size_t ws_bytes, void* stream);
size_t spr_tn_product_f64_workspace_bytes(long rows, int nl, int nr);
int spr_tn_product_f64(const float* L, const float* R, long rows, int nl, int nr, float* out,
                       void* ws, size_t ws_bytes, void* stream);
int spr_reduce_parts(const float* parts, int nparts, long n, float scale, float* out,
                     int accumulate, void* stream);
int spr_act_bwd(const float* y, const float* dy, int act, long n, float* out, void* stream);
size_t spr_colsum_workspace_bytes(int n);
int spr_colsum(const float* x, long m, int n, float* out, void* ws, size_t ws_bytes, void* stream);
size_t spr_layernorm_bwd_workspace_bytes(int c);
int spr_layernorm_bwd(const float* x, int m, int c, const float* gamma, float eps,
                      const float* dy_norm, const float* dy_pos, float* dx, float* dgamma,
                      float* dbeta, void* ws, size_t ws_bytes, void* stream);
size_t spr_instnorm_bwd_workspace_bytes(int max_len_host, int nb, int c);
int spr_instnorm_bwd(const float* x, const float* out, const float* dout, const int* cu, int n,
                     int nb, int max_len_host, int c, float eps, int norm, float slope,
                     float* dx, float* dadd, void* ws, size_t ws_bytes, void* stream);
/* The three scatter-adds of the backward (max-pool, row gather, KPConv neighbour gather) sum in 64-bit
 * fixed point with integer atomics -- order independent, bitwise reproducible -- and WRITE dx in full
 * (no pre-zeroing); ws: spr_scatter_workspace_bytes(rows of dx, channels). */
size_t spr_scatter_workspace_bytes(long rows, int c);
int spr_maxpool_bwd(const float* x, int ns, int c, const int* idx, int nq, int idx_stride, int k,
                    const float* dy, float* dx, void* ws, size_t ws_bytes, void* stream);
int spr_scatter_rows_add(const float* dy, const int* idx, int n, int c, int n_src, float* dx,
                         void* ws, size_t ws_bytes, void* stream);
size_t spr_kpconv_weighted_features_workspace_bytes(int ns);
int spr_kpconv_weighted_features(const float* q_xyz, int nq, const float* s_xyz, int ns,
                                 const int* nbr, int nbr_stride, int kmax, const float* x, int cin,
                                 const float* kernel_points, int n_kp, float kp_extent,
                                 float* wf, float* cnt, void* ws, size_t ws_bytes, void* stream);
int spr_kpconv_bwd_dx(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr,
                      int nbr_stride, int kmax, int cin, const float* kernel_points, int n_kp,
                      float kp_extent, const float* dwf, const float* dwf_range, int dwf_range_n, float* dx,
                      void* ws, size_t ws_bytes, void* stream);
int spr_softmax_rows(float* mat, const void* desc_dev, int nbatch, int max_m, void* stream);
int spr_softmax_bwd_rows(const float* p, float* dp, const void* desc_dev, int nbatch, int max_m,
                         void* stream);

/* Loss and pose-head gradients.
 * spr_bce_logits_mean_bwd: dx = gout[0] (sigmoid(x) - y) / n.
 * spr_infonce_pair_dlogits: recomputes the pair's logits and writes the un-normalised
 *   d logits [n, m] + row mask [n] (divide by sum(mask)); also returns W_sym [d, d] and
 *   t = A W_sym [n, d] for the caller's GEMM chain; spr_wsym_bwd maps d W_sym to d W.
 * spr_transform_l1_pair_bwd: d pose_pred [3,4] of spr_transform_l1_pair.
 * spr_weighted_procrustes_bwd: gradient of the Kabsch solve w.r.t. b, w (and a if da != NULL)
 *   by implicit differentiation of the SVD-based rotation (se3_torch.py:141-162; the reference
 *   uses torch.svd's autograd).  da / db / dw packed like a / b / w.
 * spr_sinkhorn_bwd: gradient of spr_sinkhorn_correspondences w.r.t. feat, alpha, beta
 *   (unrolled over the n_iters slack-Sinkhorn iterations; se3_torch.py:166-239,
 *   qk_regtr_full.py:525-536).
 */
int spr_bce_logits_mean_bwd(const float* x, const float* y, int n, const float* gout, float* dx,
                            void* stream);
int spr_infonce_pair_dlogits(const float* anchor_feat, int n, const float* positive_feat, int m,
                             int d, const float* anchor_xyz, const float* pose_gt,
                             const float* positive_xyz, const float* W, float r_p, float r_n,
                             float* dlogits, float* row_mask, float* wsym_out, float* t_out,
                             void* ws, size_t ws_bytes, void* stream);
int spr_wsym_bwd(const float* dwsym, int d, float* dW, void* stream);
int spr_transform_l1_pair_bwd(const float* pose_gt, const float* pose_pred, const float* xyz, int n,
                              const float* gout, float* dpose_pred, void* stream);
int spr_weighted_procrustes_bwd(const float* a, const float* b, const float* w,
                                const int* pair_cu, int npairs, const float* dpose, float* da,
                                float* db, float* dw, void* stream);
size_t spr_sinkhorn_bwd_workspace_bytes(const int* cu_host, int npairs, int n_iters);
int spr_sinkhorn_bwd(const float* feat, int d, const float* xyz, const int* cu,
                     const int* cu_host, int npairs, const float* alpha, const float* beta,
                     int n_iters, const float* dw, const float* dthat, float* dfeat,
                     float* dalpha, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* Circle feature loss (CircleLossFull, dist_type 'euclidean': models/losses/feature_loss.py:160-243;
 * feature_loss_type: circle, qk_regtr_full.py:91-96), all pairs of a step in one set of launches.
 * src_feat [sum N, d] / tgt_feat [sum M, d] (16-byte aligned, d % 4 == 0), src_xyz [sum N, 3] (transformed
 * by pose_gt [nbatch, 3, 4] inside), tgt_xyz [sum M, 3]; pair b owns rows cu_src[b] .. cu_src[b + 1] and
 * cu_tgt[b] .. cu_tgt[b + 1] (DEVICE int32 [nbatch + 1]); max_n / max_m bound every pair's sizes.
 * spr_circle_loss: out[b] = the pair's loss (NaN if no row or no column has both a positive and a
 *   negative, as the reference's empty mean).  Masked and zero-weight entries have logit 0.
 * spr_circle_loss_bwd: given gout[nbatch] = d L / d out, writes G[b][i][j] (row stride max_m, pair stride
 *   max_n * max_m) = (d L / d fd_ij) / fd_ij and initialises d_src = rowsum(G) src_feat, d_tgt =
 *   colsum(G) tgt_feat; the gradients are complete after d_src -= G tgt_feat and d_tgt -= G^T src_feat
 *   (two spr_bgemm calls, alpha -1, beta 1).
 * Deterministic (fixed-order float64 merges, no atomics).  ws: spr_circle_loss_workspace_bytes. */
size_t spr_circle_loss_workspace_bytes(int nbatch, int max_n, int max_m);
int spr_circle_loss(const float* src_feat, const float* tgt_feat, int d, const float* src_xyz,
                    const float* pose_gt, const float* tgt_xyz, const int* cu_src, const int* cu_tgt,
                    int nbatch, int max_n, int max_m, float r_p, float r_n, float* out, void* ws,
                    size_t ws_bytes, void* stream);
int spr_circle_loss_bwd(const float* src_feat, const float* tgt_feat, int d, const float* src_xyz,
                        const float* pose_gt, const float* tgt_xyz, const int* cu_src, const int* cu_tgt,
                        int nbatch, int max_n, int max_m, float r_p, float r_n, const float* gout, float* G,
                        float* d_src, float* d_tgt, void* ws, size_t ws_bytes, void* stream);

/* Per-launch timing of the fused KPConv kernel and of the attention core kernel
 * with HIP events recorded on the launch stream (used by bench.py for the
 * roofline figures; off by default).
 * spr_prof_enable(1) clears the log and starts recording, spr_prof_enable(0)
 * clears and stops.  spr_prof_read synchronises on the recorded events, CONSUMES them and
 * returns up to max_records entries (all arrays HOST memory):
 *   codes[i] = cin * 100000 + cout (KPConv) or -1 (attention core), nqs[i] =
 *   query / token count, ms[i] = duration. */
int spr_prof_enable(int on);
int spr_prof_read(int max_records, int* codes_host, int* nqs_host, float* ms_host);

/* MFMA / wave layout self test (writes 0 to *status_host on success). */
int spr_selftest(int* status_host);

#ifdef __cplusplus
}
#endif
#endif /* SPR_H_ */
