/*
 * gcl_amd.h -- C ABI of libgcl_hip.so, the MI355X (gfx950) native library under the
 * MinkowskiEngine-compatible operator surface used by liuQuan98/GCL's hot path.
 *
 * Boundary.  The reference reaches its native code only through the third-party
 * Python module `MinkowskiEngine` (model/resunet.py:3-4); the entry points below are what that module's
 * native half has to provide for the calls the reference makes:
 *
 *   ME.SparseTensor(feats, coordinates=...)          lib/colocation_trainer.py:843-845,
 *                                                    scripts/test_kitti.py:143-147, util/misc.py:128
 *        -> gcl_coords_insert                        (coordinate map of the stride-1 tensor)
 *   ME.MinkowskiConvolution / ...Transpose           model/resunet.py:38-171, model/residual_block.py:23-33
 *        -> gcl_stride_map, gcl_kernel_map, gcl_kernel_map_pairs   (coordinate manager, cached per key)
 *        -> gcl_pack_weights, gcl_conv_fwd (forward AND input-gradient), gcl_conv_bwd_weight,
 *           gcl_stem_fwd / gcl_stem_bwd_weight       (Cin <= 4 first layer, model/resunet.py:38-45)
 *   ME.MinkowskiBatchNorm + MEF.relu + `out += residual`   model/common.py:4-6, model/residual_block.py:37-53
 *        -> gcl_bn_stats, gcl_bn_apply, gcl_bn_bwd_reduce, gcl_bn_bwd_apply
 *   ME.MinkowskiInstanceNorm (every cloud on its own)   model/common.py:7-8, model/resunet.py:269-291
 *        -> gcl_in_fwd, gcl_in_bwd
 *   out.F / torch.norm(out.F, p=2, dim=1, keepdim=True)   model/resunet.py:226-230  -> gcl_row_normalize_fwd/bwd
 *   finest_contrastive_loss                          lib/colocation_trainer.py:430-535
 *        -> gcl_group_loss_fwd/bwd, gcl_nn_rowmin (pdist + min, lib/metrics.py:22-25),
 *           gcl_neg_mask, gcl_neg_loss_fwd/bwd
 *   find_nn_gpu                                      lib/eval.py:18-48  -> gcl_nn_rowmin
 *   Matcher.estimator (SC2-PCR)                      scripts/test_kitti.py:172-180, scripts/SC2_PCR/SC2_PCR.py
 *        -> gcl_nn_rowmin, gcl_sc2_*
 *   open3d registration_ransac_based_on_feature_matching   scripts/test_kitti.py:171-178,
 *                                                    generalization_ETH/evaluate.py:171-186
 *        -> gcl_nn_rowmin, gcl_ransac_register, gcl_ransac_register_batch, gcl_mutual_correspondences
 *   find_nearest_voxel_feature, calculate_M, inlier ratio   generalization_ETH/evaluate.py:63-77, :110-122, :160-169
 *        -> gcl_nn3_rowmin, gcl_nn_rowmin, gcl_mutual_match; a scene's logged pairs in chunks: gcl_nn_rowmin_batch,
 *           gcl_mutual_match_batch
 *   eval_KITTI_per_pair, eval_3DMatch_scene (SC2-PCR benchmark)   scripts/SC2_PCR/test_KITTI.py:18-85,
 *                                                    test_3DMatch.py:18-76, evaluate_metric.py
 *        -> gcl_nn_rowmin / gcl_nn_rowmin_any (any descriptor width), gcl_sc2_register_batch, gcl_registration_stats;
 *           a chunk's searches and correspondence gathers in one call: gcl_nn_rowmin_batch (with the mutual filter:
 *           gcl_mutual_correspondences_batch)
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless its name ends in _host;
 *   - the caller owns all memory (the Python host allocates torch tensors); the library never allocates
 *     persistent device memory and never synchronises the stream;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - return 0 on success, <0 on error; gcl_last_error() gives the message of the calling thread's last error;
 *   - row-major contiguous matrices; features are fp32, indices int32, coordinates int32 [N,4] = (batch,x,y,z).
 */
#ifndef GCL_AMD_H
#define GCL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCL_OK 0
#define GCL_ERR_ARG (-1)       /* bad argument (shape not supported, null pointer, ...) */
#define GCL_ERR_HIP (-2)       /* a HIP runtime call failed */
#define GCL_ERR_NO_DEVICE (-3) /* no gfx950 device visible */

#define GCL_PAIR_CHUNK 128     /* pair lists are padded per kernel offset to a multiple of this */

const char* gcl_last_error(void);
int gcl_version(void);
/* number of visible devices, or <0; never throws -- used by the host to fail loudly without a GPU */
int gcl_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Coordinate maps.  A map is an open-addressing hash table the CALLER allocates:
 *   table: int64 [cap, 2]  (slot = {packed key, row index}), cap = power of two >= 2 * n.
 * Keys pack (batch, x, y, z) into 16 bits each (x,y,z offset by 2^15).
 * status (int32[4], device): [0] = #rows with a coordinate outside the packable range,
 *                            [1] = #duplicate rows met by gcl_coords_insert.
 * ---------------------------------------------------------------------------------------------- */
int gcl_coords_insert(const int32_t* coords, int64_t n, int64_t* table, int64_t cap,
                      int32_t* status, void* stream);

/* Strided coordinate map: out = unique(floor(c / t_out) * t_out), rows ordered by first occurrence in
 * `coords_in` (deterministic).  Writes coords_out (capacity n_in rows), n_out_dev (device int32) and
 * fills `table_out` (cap_out >= 2 * n_in) with out-key -> out-row.  scratch: int32[gcl_scan_scratch_len(n_in)].
 * n_in_dev (optional, device int32): the true row count when n_in is only an upper bound -- lets the host chain
 * the maps of several levels without reading a count back in between. */
int64_t gcl_scan_scratch_len(int64_t n);
int gcl_stride_map(const int32_t* coords_in, int64_t n_in, const int32_t* n_in_dev, int32_t t_out,
                   int64_t* table_out, int64_t cap_out, int32_t* scratch,
                   int32_t* coords_out, int32_t* n_out_dev, int32_t* status, void* stream);

/* Device-wide exclusive prefix sum of int32 (scratch: int32[n / 2048 + 64]); used by the map builders. */
int gcl_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * "Next" rows: the loader work either side of the hot path, on the device.
 * gcl_voxel_coords + gcl_unique_coords = ME.utils.sparse_quantize(xyz / voxel, return_index=True)
 *   (util/misc.py:117-118, lib/colocation_data_loader.py:379,388): coords = floor(xyz / voxel) (correctly rounded
 *   fp32 division, floor toward -inf), one row per voxel = first occurrence, kept rows in ascending order;
 *   index_out[j] = input row of output row j; table_out maps the kept coordinates to their output rows.
 * gcl_colocation_hits + gcl_colocation_emit = get_matching_indices_colocation (util/pointcloud.py:69-132):
 *   xyz_own [Ntot,3]: voxel-representative points of the centre cloud followed by the neighbour clouds, each in its
 *   OWN sensor frame; xyz_cf: the same points in the CENTRE frame (neighbours transformed by list_M, fp32);
 *   table: coordinate map of floor(xyz_own / voxel) with batch id = cloud id; to_cloud_host: double[n_clouds][12],
 *   row-major 3x4 transforms centre frame -> cloud frame (identity for cloud 0), used only to find candidate voxels.
 *   hits [n_center, n_clouds, K] (rows into xyz_*, ascending distance, -1 padded), cnt, first_rng: per (centre point,
 *   cloud).  emit: group [G], index [sum], finest [sum] (exactly one 1 per group), totals = {G, sum} on the device.
 * ---------------------------------------------------------------------------------------------- */
int gcl_voxel_coords(const float* xyz, int64_t p, float voxel, int32_t batch_id, int32_t* coords, void* stream);
int gcl_unique_coords(const int32_t* coords_in, int64_t n_in, int64_t* table_out, int64_t cap_out, int32_t* scratch,
                      int32_t* coords_out, int64_t* index_out, int32_t* n_out_dev, int32_t* status, void* stream);
int gcl_colocation_hits(const float* xyz_own, const float* xyz_cf, int64_t n_center, int32_t n_clouds,
                        const double* to_cloud_host, const int64_t* table, int64_t cap, float inv_voxel, double radius,
                        int32_t K, int32_t* hits, int32_t* cnt, double* first_rng, void* stream);
int gcl_colocation_emit(const int32_t* hits, const int32_t* cnt, const double* first_rng, int64_t n_center,
                        int32_t n_clouds, int32_t K, int32_t* scratch, int32_t* group, int64_t* index, uint8_t* finest,
                        int32_t* totals, void* stream);

/* A whole BATCH of samples in one pass (round 6; what ColocationKittiDataset.__getitem__ x batch_size + collate_colocation_fn
 * produce, lib/colocation_data_loader.py:315-475): the clouds of ALL samples share ONE coordinate table whose batch id is the
 * cloud's number in the batch (the ids sparse_collate gives them, :440-446), so a batch costs two host synchronisations.
 *   gcl_voxel_coords_multi  gcl_voxel_coords over the concatenated points of n_clouds <= 64 clouds; cloud_offsets_host:
 *                           HOST int64[n_clouds + 1] point offsets (offsets[0] = 0, offsets[n_clouds] = p).
 *   gcl_cloud_row_starts    after gcl_unique_coords (rows keep the cloud-major input order): starts int32[n_clouds + 1] on the
 *                           device, starts[c] = first row of cloud c (-1: the cloud has none), starts[n_clouds] = *n_dev.
 *   gcl_loader_points       voxel representatives xyz_own[i] = xyz_raw[index[i]] and, in the centre frame of the row's sample,
 *                           xyz_cf[i] = fp32(R p + t) evaluated in fp64 without contraction; to_center_dev: DEVICE
 *                           double[n_clouds][12] (row-major 3 x 4; identity for a centre cloud).  n_max bounds the launch,
 *                           *n_dev rows are written.
 *   gcl_colocation_hits_at  gcl_colocation_hits for ONE sample of the batch: its centre voxels are rows row0 .. row0 + n_center
 *                           of xyz_*, its clouds are the table's batch ids cloud0 .. cloud0 + n_clouds - 1; hits are rows of
 *                           the batch (= the `index` collate_colocation_fn makes by adding the sample's offset, :434-437).
 *                           hits / cnt / first_rng point at the sample's slice; gcl_colocation_emit then runs once over the
 *                           concatenated centre voxels of all samples. */
int gcl_voxel_coords_multi(const float* xyz, int64_t p, const int64_t* cloud_offsets_host, int32_t n_clouds, float voxel,
                            int32_t* coords, void* stream);
int gcl_cloud_row_starts(const int32_t* coords, int64_t n_max, const int32_t* n_dev, int32_t n_clouds, int32_t* starts,
                         void* stream);
int gcl_loader_points(const float* xyz_raw, const int64_t* index, const int32_t* coords, int64_t n_max, const int32_t* n_dev,
                      const double* to_center_dev, float* xyz_own, float* xyz_cf, void* stream);
int gcl_colocation_hits_at(const float* xyz_own, const float* xyz_cf, int64_t row0, int64_t n_center, int32_t cloud0,
                           int32_t n_clouds, const double* to_cloud_host, const int64_t* table, int64_t cap, float inv_voxel,
                           double radius, int32_t K, int32_t* hits, int32_t* cnt, double* first_rng, void* stream);

/* The loader's augmentation on the device (lib/colocation_data_loader.py:349-370, lib/data_loaders.py:476-492): every cloud
 * turned about its centroid, the sample's scale applied, inside the two passes above that touch every point.
 *   gcl_cloud_centroids     centroids double[n_clouds][3] of the clouds of gcl_voxel_coords_multi's layout: fp64 sums of the fp32
 *                           points in a fixed order (no atomics) / the number of points; bitwise the same for a cloud alone,
 *                           anywhere in any batch and on every run; zeros for an empty cloud.  scratch: device
 *                           double[gcl_cloud_centroids_scratch_len(p, n_clouds)].
 *   gcl_cloud_affines       aff double[n_clouds][12] (row-major 3 x 4) = T_c = [R_c | R_c (-centroid_c)], every dot product
 *                           ((a b + c d) + e f) in fp64, uncontracted.  aug_dev: DEVICE double[n_clouds][12] = R_c (9, row-major),
 *                           the scale (1.0: none), rotated (0.0 / 1.0), one spare; a cloud with rotated = 0 gets [I | 0].
 *   gcl_voxel_coords_aug    gcl_voxel_coords_multi of the augmented points.  mode 1 (f32, the co-location loaders): T_c rounded
 *                           to fp32, y = (((x0 r0 + x1 r1) + x2 r2) + t) * fp32(scale) in fp32, floor(y / fp32(voxel)); mode 2
 *                           (f64, the pair loaders): y = scale * (((x0 r0 + x1 r1) + x2 r2) + t) in fp64, floor(y / voxel) by
 *                           fp64 division.  A cloud with rotated = 0 is y = x * fp32(scale) in fp32 in both modes.
 *   gcl_loader_points_aug   gcl_loader_points with xyz_own[i] = that y (mode 2: fp32(y)) of point index[i]; xyz_cf from xyz_own. */
int64_t gcl_cloud_centroids_scratch_len(int64_t p, int32_t n_clouds);
int gcl_cloud_centroids(const float* xyz, int64_t p, const int64_t* cloud_offsets_host, int32_t n_clouds, double* scratch,
                        double* centroids, void* stream);
int gcl_cloud_affines(const double* aug_dev, const double* centroids, int32_t n_clouds, double* aff_dev, void* stream);
int gcl_voxel_coords_aug(const float* xyz, int64_t p, const int64_t* cloud_offsets_host, int32_t n_clouds, double voxel,
                         const double* aug_dev, const double* aff_dev, int32_t mode, int32_t* coords, void* stream);
int gcl_loader_points_aug(const float* xyz_raw, const int64_t* index, const int32_t* coords, int64_t n_max, const int32_t* n_dev,
                          const double* to_center_dev, const double* aug_dev, const double* aff_dev, int32_t mode,
                          float* xyz_own, float* xyz_cf, void* stream);

/* HOST function (no GPU, every pointer is a HOST pointer): numpy's legacy np.random.choice(n, k, replace=False) =
 * permutation(n)[:k] -- the three draws of every training step (lib/colocation_trainer.py:457, :506-507) -- reproduced
 * bit for bit from the RandomState's MT19937 state (key[624], *pos as in np.random.get_state(); both updated in place so
 * that np.random.set_state continues the stream), outside the interpreter lock: numpy needs 8 ms per call at 0.5 M rows and
 * holds the lock meanwhile, which stalls the thread that enqueues the GPU work.  work: int64[n + n / 32 + 64] scratch,
 * out: int64[k]. */
int gcl_host_legacy_choice(uint32_t* key, int32_t* pos, int64_t n, int64_t k, int64_t* work, int64_t* out);

/* Ground-truth correspondences of scan pairs = get_matching_indices (util/pointcloud.py:53-66; called by every pair dataset,
 * lib/data_loaders.py:256, :506), for a ragged batch of n_pairs >= 1 pairs in the launches of one: count, scan, emit.
 *   xyz0 [total0, 3], offsets0 int64 [n_pairs + 1]   the source points (one per voxel), pair b = rows offsets0[b] .. offsets0[b+1]
 *   xyz1 [total1, 3], offsets1 int64 [n_pairs + 1]   the target points, likewise            (all of these on the DEVICE)
 *   table, cap        coordinate hash table that holds floor(xyz1 / voxel) of every target under the batch id
 *                     cloud0 + b * cloud_stride (gcl_unique_coords / gcl_coords_insert make it; other clouds may live in it)
 *   table_row0        int64 [n_pairs] or NULL: the table's value of target b's FIRST row (the table may number the rows of a
 *                     larger array, e.g. all 2 B clouds of a batch); NULL = offsets1[b], the values address xyz1 directly
 *   voxel             the voxel size the table's coordinates were made with (the query's voxel is q / voxel in fp64)
 *   trans             double [n_pairs][12], row-major 3 x 4: source -> target frame;  radii: double [n_pairs]
 *   radius_max        HOST bound of the radii: radius_max / voxel >= 4 (more than 9^3 candidate voxels) returns GCL_ERR_ARG
 *                     before anything is launched
 *   K                 keep the first K hits of a source row; 0 = all (the reference's K = None)
 * Arithmetic (that of gcl_colocation_hits): q = ((x m0 + y m1) + z m2) + t in fp64 from the fp32 point; d2 = ((ex^2 + ey^2) +
 * ez^2) against the fp32 target point; a hit is d2 < r r; a row's hits are ordered by (d2, j); output by i, then that order.
 * gcl_pair_matches_count   cnt int32 [total0] = kept hits per source row; scratch: int32 [gcl_pair_matches_scratch_len(total0)]
 *                          (row offsets, read again by emit); meta: DEVICE int64 [2 + n_pairs] = {P, status, matches of pair
 *                          0, 1, ...}.  status 1: offsets not 0 <= o[b] <= o[b+1] <= total; 2: a radius not in (0, radius_max];
 *                          then nothing but the status word is written, by either call.
 * gcl_pair_matches_emit    pairs int64 [n_matches, 2], n_matches = the P the host read from meta; absolute = 0: rows relative
 *                          to the pair's own clouds, 1: rows of xyz0 / xyz1 (collate_pair_fn's running start indices added,
 *                          lib/data_loaders.py:52-57).  Same inputs as the count call. */
int64_t gcl_pair_matches_scratch_len(int64_t total0);
int gcl_pair_matches_count(const float* xyz0, int64_t total0, const int64_t* offsets0, const float* xyz1, int64_t total1,
                           const int64_t* offsets1, const int64_t* table_row0, int32_t n_pairs, const int64_t* table,
                           int64_t cap, int32_t cloud0, int32_t cloud_stride, float voxel, const double* trans,
                           const double* radii, double radius_max, int32_t K, int32_t* cnt, int32_t* scratch, int64_t* meta,
                           void* stream);
int gcl_pair_matches_emit(const float* xyz0, int64_t total0, const int64_t* offsets0, const float* xyz1, int64_t total1,
                          const int64_t* offsets1, const int64_t* table_row0, int32_t n_pairs, const int64_t* table,
                          int64_t cap, int32_t cloud0, int32_t cloud_stride, float voxel, const double* trans,
                          const double* radii, double radius_max, int32_t K, int32_t absolute, const int32_t* scratch,
                          const int64_t* meta, int64_t* pairs, int64_t n_matches, void* stream);

/* Kernel map for kernel size ks^3 (x fastest in k), offsets scaled by `step` (= input tensor stride x dilation),
 * region centred on the OUTPUT coordinate:  nbr[k * n_out + v] = input row at c_out[v] + o_k * step, or -1.
 * same_map != 0: coords_out IS the input map (stride-1 conv): only offsets k <= K/2 are looked up, the mirror
 *   entries nbr[(K-1-k) * n + u] = v are written from the hits; nbr_t must be NULL.
 * same_map == 0 and nbr_t != NULL (n_in rows): nbr_t[k * n_in + u] = v for every pair (filled with -1 first).
 * same_map bit 1 (value 2): `bitmap` was already filled for THIS table_in by an earlier call (the three kernel maps that
 *   read the stride-1 table of a step share one fill); bit 0 is the same-map flag described above.
 * same_map bit 2 (value 4): `counts` is ZERO on entry (gcl_maps_build zeroes every map's counts with one fill): builds of
 *   <= 64 blocks (16 384 output rows) then add their per-block counts with integer atomics -- the same totals, one launch
 *   less per map, `scratch` unused; longer builds take the ordered reduction as before (the counters share two cache lines).
 * same_map bit 3 (value 8): nbr (and nbr_t) hold -1 in EVERY entry on entry (gcl_maps_build pre-fills the tables of a small
 *   build with one launch): the call's own fills are skipped.
 * bitmap: optional int32[gcl_kernel_map_bitmap_len()] scratch: a presence bit per hashed key lets most absent
 *   neighbours return without probing the table.  scratch: int32[gcl_kernel_map_scratch_len(ks, n_out)] (per-block
 *   pair counts, summed in order -- no contended atomics).  counts[k] (int32[K], device) = #pairs of offset k. */
int64_t gcl_kernel_map_bitmap_len(void);
int64_t gcl_kernel_map_scratch_len(int32_t ks, int64_t n_out);
int gcl_kernel_map(const int32_t* coords_out, int64_t n_out, const int64_t* table_in, int64_t cap_in,
                   int32_t ks, int32_t step, int32_t same_map, int32_t* bitmap, int32_t* scratch, int32_t* nbr,
                   int32_t* nbr_t, int64_t n_in, int32_t* counts, void* stream);

/* Compact per-offset pair lists from nbr (out-major, ascending out row inside an offset), each offset's
 * segment padded with -1 to a multiple of GCL_PAIR_CHUNK:
 *   seg_off_host: int64[K+1] HOST array computed by the caller from `counts` (padded prefix sums);
 *   pair_in / pair_out: int32[seg_off_host[K]].  scratch: int32[K * ceil(n_out/1024) + K + 1]. */
int gcl_kernel_map_pairs(const int32_t* nbr, int32_t K, int64_t n_out, const int64_t* seg_off_host,
                         int32_t* scratch, int32_t* pair_in, int32_t* pair_out, void* stream);

/* What the map builders launch for a row count: host arithmetic, no GPU (gcl_stride_map / gcl_unique_coords,
 * gcl_kernel_map, gcl_kernel_map_pairs and gcl_maps_build call the same function; tests place their cases on both sides
 * of every limit with it).  n = the row count the entry dispatches on (n_in of a strided level, n_out of a kernel map and
 * of its pair lists, the input rows of gcl_maps_build); ks, same_map as for gcl_kernel_map.
 * out = {strided level: 1 = long form (flags, three-launch scan, emit), 0 = short form; its scan blocks;
 *        kernel map: counts by integer atomics; grid x; grid y; the count reduction is launched (over grid x blocks);
 *        pair lists: compaction blocks; gcl_maps_build: one -1 fill for all tables; a presence bitmap per table;
 *        offsets per thread of the lookup kernels; 0; 0}. */
int gcl_map_launch_shape(int64_t n, int32_t ks, int32_t same_map, int32_t out[12]);

/* Row ordering for the output-stationary convolution: sorts the rows of a [K][n] neighbour table (K <= 27) by
 * their K-bit presence mask (stable radix sort), so that the rows of a 32-row wave tile need nearly the same offsets.
 * The sort key is the mask with its bits re-ordered by how often each offset occurs in THIS table -- the
 * rarest offset is the most significant key bit, the most frequent the least significant, ties: lower offset lower --
 * and the sort runs on the key's 24 most significant bits (key >> max(0, K - 24), three 8-bit passes).  Rows that own a
 * rare offset then share its visit.  The convolution walks the tiles from the END of this order (the tiles with the
 * most offsets first).  order[j] = original row at sorted position j; tbl_sorted[k*n + j] = tbl[k*n + order[j]];
 * tile_mask[t] = OR of the masks of sorted rows 32t .. 32t+31.  scratch: int32[gcl_table_sort_scratch_len(n)].
 * gcl_table_sort is gcl_table_sort_multi with one job without `counts`. */
int64_t gcl_table_sort_scratch_len(int64_t n);
int gcl_table_sort(const int32_t* tbl, int32_t K, int64_t n, int32_t* scratch, int32_t* order, int32_t* tbl_sorted,
                   int32_t* tile_mask, void* stream);
/* The mask sort of SEVERAL tables in one sequence of 14 launches (a network has 12 such tables: 168 launches one by
 * one).  Same results bit for bit.  All tables of a call share K. */
typedef struct gcl_sort_job {
  const int32_t* tbl;
  int32_t K;
  int64_t n;
  int32_t* scratch;      /* int32[gcl_table_sort_scratch_len(n)] */
  int32_t* order;
  int32_t* tbl_sorted;
  int32_t* tile_mask;
  const int32_t* counts; /* optional int32[K], device: rows per offset (= gcl_kernel_map's counts, for nbr and for nbr_t alike);
                            when EVERY table of the call has it the bit-count and key passes fold into the first launch */
} gcl_sort_job;
int gcl_table_sort_multi(const gcl_sort_job* jobs_host, int32_t n_jobs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse convolution (fp32, exact-f32 MFMA).
 * gcl_pack_weights: W [K, Cin, Cout] -> MFMA B-fragment order.
 *   mode 0: forward weights            (Cin_eff = Cin,  Cout_eff = Cout, k kept)
 *   mode 1: transposed per offset      (Cin_eff = Cout, Cout_eff = Cin,  k kept)     input-gradient, in != out map
 *   mode 2: transposed + offsets mirrored (k -> K-1-k)                               input-gradient, same map
 *   prec 0: exact-f32 MFMA (v_mfma_f32_32x32x2_f32), wp = float[K * Cin * Cout];
 *   prec 3: fp32 operands split into 3 bf16 planes, 6 bf16-MFMA terms, fp32 accumulate ("bf16x6": error vs fp64
 *           equal to native fp32, 2.7x the MFMA rate);  prec 2: 2 planes, 3 terms ("bf16x3", ~1.5e-5, 5.3x);
 *   prec 4: 2 fp16 planes of the operands scaled by a per-tensor power of two (gcl_amax), 3 fp16-MFMA terms
 *           ("fp16x3": 11+11 significand bits with round-to-nearest = 24 bits, i.e. native-fp32 accuracy at half the
 *           MFMA work of bf16x6); x_amax / w_amax are required in this mode only;
 *           wp = gcl_pack_weights_bytes(...) bytes of bf16 planes.
 *   Shapes: the MFMA kernels take Cin, Cout multiples of 32 and K <= 27.  EVERY OTHER shape (any Cin, Cout > 0, K <= 125;
 *   e.g. the 16-dim head of demo.py:29, `final` 64 -> 16) is a "generic shape": gcl_pack_weights then writes plain fp32
 *   W_eff[k][Cin_eff][Cout_eff] (prec ignored), gcl_conv_fwd / gcl_conv_fwd_fused / gcl_conv_bwd_weight run exact-fp32
 *   VALU kernels (amax pointers, plane images and `stats` are not used / not accepted there).
 *   The generic weight gradient accumulates and keeps its per-workgroup slabs in fp64 and rounds once (with Ca = Cb = 1 a
 *   dW[k] is one sum of products of either sign); gcl_conv_bwd_weight_scratch_len accounts for it.
 * gcl_conv_fwd: Y[row(j)] = sum_k X[tbl[k*n_out+j]] . Wp_k (+ bias); tbl == NULL means K == 1, identity.
 *   x_is_planes != 0 (prec 4 only): x points at the gcl_split_planes image of X instead of X (no split in the kernel).
 *   X has n_in rows (n_in * Cin * 4 < 4 GiB: rows are gathered through a buffer resource, absent neighbours read 0).
 *   With (order, tile_mask) from gcl_table_sort, `tbl` is the PERMUTED table, row(j) = order[j] and each 32-row
 *   wave tile visits only the offsets of tile_mask; with NULLs, row(j) = j and every offset is visited.
 *   Output-stationary (no atomics, deterministic).  The same entry computes the input gradient when given
 *   the opposite table and mode-1/2 weights.  K <= 27.
 *   stats (optional, split precisions): float[4][cout][ceil(n_out/128)] (channel-major) -- column sums of y and y^2,
 *   column minimum and maximum per 128-row workgroup tile (its four waves combined in order), consumed by
 *   gcl_bn_stats_from_tiles(_range) (the BatchNorm that follows then needs no statistics pass over y; n_tiles =
 *   ceil(n_out/128), its `scratch` is unused). */
int64_t gcl_pack_weights_bytes(int32_t K, int32_t cin, int32_t cout, int32_t prec);
/* max |x| of a tensor in an "amax slot": GCL_AMAX_WORDS device int32, 16 entries on separate 128-byte lines (entry i
 * at word 32 i), value = max over the entries, each the bit pattern of a non-negative float.  (Workgroups publish to
 * different lines: same-line atomics serialise on gfx950.)  The fp16x3 mode derives its exact power-of-two operand
 * scales from it.  zeroed != 0: the caller guarantees the slot is all zero on the stream (slots handed out from a
 * zero-filled pool), so no memset is issued. */
#define GCL_AMAX_WORDS 512
int gcl_amax(const float* x, int64_t n, int32_t* amax_bits, int32_t zeroed, void* stream);
/* gcl_amax of n_tensors tensors in one launch: ptrs / sizes are DEVICE arrays (float* and element counts),
 * amax_bits[n_tensors * GCL_AMAX_WORDS] (one slot per tensor) is cleared here.  Used once per step for all convolution kernels of a model. */
int gcl_amax_multi(const float* const* ptrs, const int64_t* sizes, int32_t n_tensors, int32_t* amax_bits,
                   void* stream);
int gcl_pack_weights(const float* w, int32_t K, int32_t cin, int32_t cout, int32_t mode, int32_t prec,
                     const int32_t* w_amax, void* wp, void* stream);
/* gcl_pack_weights for a list of tensors in ONE launch (all convolution kernels of a network, once per optimizer step
 * and direction).  desc: DEVICE int64[n_tensors][8] = {w pointer, K, cin, cout, mode, amax slot index, byte offset of
 * the packed tensor inside `out`, first workgroup}, first workgroup = running sum of ceil(K*cin*cout / 256);
 * total_wgs = that sum over all tensors; amax_slots: the slots written by gcl_amax_multi (prec 4).  prec 2, 3 or 4. */
int gcl_pack_weights_multi(const int64_t* desc, int32_t n_tensors, int64_t total_wgs, int32_t prec,
                           const int32_t* amax_slots, void* out, void* stream);
/* NB of the kernel instance gcl_conv_fwd will launch for this shape (a wave covers 32 NB output columns): 4, 2 or 1;
 * diagnostic (profile labels). */
int32_t gcl_conv_fwd_nb(int64_t n_out, int32_t cout, int32_t prec);
/* fp16x3 operand image of an activation tensor: planes = uint16 [n][c / 32][2][32] -- per row and 32-channel slice the
 * fp16 hi values (64 bytes) then the fp16 lo values (64 bytes) of x * scale(amax), i.e. 4 bytes per element like x.
 * A tensor that several launches consume (forward, weight gradient; input gradient, weight gradient) is split once. */
int gcl_split_planes(const float* x, int64_t n, int32_t c, const int32_t* amax, void* planes, void* stream);
/* flags: GCL_CONV_XCD_RANGES -- for a table whose row order is spatially coherent: give every XCD (L2) a CONTIGUOUS
 * range of row tiles, so that the input rows a tile gathers are mostly the ones its neighbours on the same XCD just
 * gathered.  Launch-order hint only. */
#define GCL_CONV_XCD_RANGES 1
#define GCL_CONV_TALL 4     /* inference launches: sixteen waves per workgroup, a tile's offsets in four FIXED groups (k with
                               k mod 4 == g) whose partial sums are added in group order -- shortens the chain of dependent
                               steps a small cloud's deep layers are made of; a row's result depends on the layer's shape only
                               (batching stays bitwise neutral).  fp16x3 on fp32 rows, no BatchNorm statistics, K >= 8,
                               K Cin / 32 >= 108 (Cin >= 128 at K = 27), Cout a multiple of 64; ignored elsewhere.  Results differ from the launch
                               without the flag in the last bits (another summation order).
                               Round 6: with this flag the `stats` argument of gcl_conv_fwd(_fused(_ld)) is SCRATCH of
                               gcl_conv_fwd_groups_scratch_len(n_out, K, Cin, Cout) floats, or NULL.  With scratch (and a
                               non-zero length: <= 65536 output rows) the four groups run as four times as many ordinary
                               workgroups + one sum / epilogue launch -- bitwise the sixteen-wave kernel's result, 2 - 3 x
                               shorter on the deep layers of a pass over one or two clouds. */
#define GCL_CONV_DMA 2      /* accepted, no effect: every fp16x3 launch stages its operands by LDS-DMA (`buffer_load ... lds`: no
                               staging registers, no ds_write) unless GCL_CONV_NO_DMA is set */
#define GCL_CONV_NO_DMA 8   /* fp16x3: the register-staged kernel for this launch; bitwise the same results */
int gcl_conv_fwd(const float* x, int64_t n_in, int32_t x_is_planes, const void* wp, int32_t prec, const int32_t* x_amax,
                 const int32_t* w_amax, const int32_t* tbl, const int32_t* order, const int32_t* tile_mask,
                 int64_t n_out, int32_t K,
                 int32_t cin, int32_t cout, const float* bias, float* y, float* stats, int32_t flags, void* stream);

/* gcl_conv_fwd with a fused inference epilogue: y = relu?(conv * col_scale + bias (+ residual)), i.e. convolution +
 * BatchNorm in eval mode (col_scale = gamma * rsqrt(var + eps), bias = beta - mean * col_scale) + BasicBlock's residual
 * add + ReLU in ONE launch (model/residual_block.py:37-53 with running statistics); y_amax (optional, zero-initialised
 * amax slot) receives max|y| for the next fp16x3 convolution.  Split-precision modes only.
 * relu == 2 (needs `residual`): aten::threshold_backward instead of the add -- y = conv where residual > 0, else 0: the
 * input gradient of a convolution whose input came out of a ReLU, with that ReLU's backward in the epilogue (`residual` =
 * the ReLU's output). */
int64_t gcl_conv_fwd_groups_scratch_len(int64_t n_out, int32_t K, int32_t cin, int32_t cout);
int gcl_conv_fwd_fused(const float* x, int64_t n_in, int32_t x_is_planes, const void* wp, int32_t prec,
                       const int32_t* x_amax, const int32_t* w_amax, const int32_t* tbl, const int32_t* order,
                       const int32_t* tile_mask, int64_t n_out, int32_t K, int32_t cin, int32_t cout, const float* bias,
                       const float* col_scale, const float* residual, int32_t relu, int32_t* y_amax, float* y,
                       float* stats, int32_t flags, void* stream);
/* the same with `residual` a column slice of a wider row-major tensor: row pitch residual_ld floats (0 = cout).  Used by the
 * backward pass for the gradient of an ME.cat input, which is a slice of the gradient of the cat's output (no split copy). */
int gcl_conv_fwd_fused_ld(const float* x, int64_t n_in, int32_t x_is_planes, const void* wp, int32_t prec,
                          const int32_t* x_amax, const int32_t* w_amax, const int32_t* tbl, const int32_t* order,
                          const int32_t* tile_mask, int64_t n_out, int32_t K, int32_t cin, int32_t cout, const float* bias,
                          const float* col_scale, const float* residual, int32_t residual_ld, int32_t relu,
                          int32_t* y_amax, float* y, float* stats, int32_t flags, void* stream);

/* What gcl_conv_fwd(_fused(_ld)) launches for a shape: host arithmetic, no GPU (the dispatcher itself calls the same
 * function after its argument checks; tests and profile labels take kernel instances from it).  x_is_planes, flags as
 * above; fused_epilogue != 0: any of col_scale, residual, relu, y_amax is given; sorted_table != 0: (order, tile_mask) are
 * given; group_scratch != 0: `stats` of a GCL_CONV_TALL launch is not NULL (ignored without that flag).
 * out = {path (GCL_FWD_PATH_*), NB (TC for the generic kernel), PL (= prec; 0 for the generic kernel), PRE + 2 EPI
 * (template arguments: plane-image operand, fused epilogue), grid x, grid y, threads per workgroup, launch-order word of
 * the kernel (bit 0: a contiguous row-tile range per XCD, bit 1: 1-D grid of ceil(tiles / 8) * 8 * column blocks with a row
 * tile's column blocks on one XCD, bit 4: mask-sorted row tiles in descending order)}. */
#define GCL_FWD_PATH_GENERIC 0  /* k_conv_generic<TC>: Cin or Cout no multiple of 32, or K > 27 */
#define GCL_FWD_PATH_F32 1      /* k_conv_fwd<NB> */
#define GCL_FWD_PATH_SPLIT 2    /* k_conv_fwd_split<NB, PL, PRE, EPI>: bf16x3, bf16x6; fp16x3 with GCL_CONV_NO_DMA */
#define GCL_FWD_PATH_DMA 3      /* k_conv_fwd_dma<NB, PRE, EPI>: fp16x3 */
#define GCL_FWD_PATH_TALL 4     /* k_conv_fwd_tall<EPI>: GCL_CONV_TALL without scratch, or more than 65536 rows */
#define GCL_FWD_PATH_GROUPS 5   /* k_conv_fwd_dma<2, false, false, true> then k_conv_groups_sum<EPI, 4>: GCL_CONV_TALL with scratch */
int gcl_conv_fwd_launch_shape(int64_t n_out, int32_t K, int32_t cin, int32_t cout, int32_t prec, int32_t x_is_planes,
                              int32_t fused_epilogue, int32_t sorted_table, int32_t group_scratch, int32_t flags,
                              int32_t out[8]);

/* dW[k] = sum over pairs of offset k of  A[pair_a]^T . B[pair_b]   (A: [*, ca], B: [*, cb]) -> dw [K, ca, cb].
 * Forward conv: A = X, pair_a = pair_in, B = dY, pair_b = pair_out.  Transposed conv: roles swapped.
 * Deterministic: per-wave partial slabs + ordered reduction.  prec as in gcl_conv_fwd (both operands are split
 * on the fly for prec 2 / 3).
 * planes != 0 (prec 4 only): a AND b point at gcl_split_planes images (no split, hardware-transposed LDS reads).
 * A has n_a rows, B n_b rows (each tensor < 4 GiB: rows are gathered through buffer resources, padding pairs read 0).
 * sorted_side: 0 = nothing known about the pair order; 1 / 2 = pair_a / pair_b ascends inside every offset segment (the
 *   out rows of gcl_kernel_map_pairs: pair_b for a forward convolution, pair_a for a transposed one).  With it, and Ca, Cb
 *   in {32, 64}, 1 < K <= 27, no plane images and >= 32768 rows on that side, the launch is "range-grouped": a workgroup
 *   takes the pairs of ONE offset whose sorted-side row lies in one row range, the K workgroups of a range share an XCD,
 *   and the sorted side's rows are fetched from the fabric once per range instead of once per offset (same sums, other
 *   fixed order).  scratch: float[gcl_conv_bwd_weight_scratch_len(K, ca, cb, n_pairs_padded, rows of the sorted side or 0)].
 * planes: bit 0 = a and b are plane images (gcl_split_planes); with Ca and Cb multiples of 128 the launch then gives every
 *   workgroup a 128 x 128 block of dW[k] whose rows are gathered once and shared by its four waves (half the gathered bytes
 *   per MFMA).  Bit 1 = keep the 64 x 64-block kernel for this launch (same result to rounding: another fixed order). */
int64_t gcl_conv_bwd_weight_scratch_len(int32_t K, int32_t ca, int32_t cb, int64_t n_pairs_padded, int64_t n_sorted_rows);
int gcl_conv_bwd_weight(const float* a, int64_t n_a, const float* b, int64_t n_b, int32_t planes, int32_t sorted_side,
                        const int32_t* pair_a, const int32_t* pair_b, const int64_t* seg_off_host, int32_t K,
                        int32_t ca, int32_t cb, int32_t prec, const int32_t* a_amax, const int32_t* b_amax, float* scratch, float* dw,
                        void* stream);
/* kernel_size-1 convolutions (conv1_tr, final: model/resunet.py:153-171; ME binds them to the same GEMM path with an
 * identity kernel map): dW[ca][cb] = sum over ALL n_rows rows of a[i][:]^T b[i][:] -- pair (i, i) for every row, so no pair
 * list is read and nothing is gathered: both operands are streamed once (k_bwd_weight_rows, fp16x3 split on the fly,
 * per-workgroup slabs summed in a fixed order: deterministic).  gcl_conv_bwd_weight_rows_scratch_len returns the scratch
 * floats, or 0 when the shape / arithmetic is not taken (then use gcl_conv_bwd_weight with identity pairs). */
int64_t gcl_conv_bwd_weight_rows_scratch_len(int32_t ca, int32_t cb, int32_t prec, int64_t n_rows);
int gcl_conv_bwd_weight_rows(const float* a, const float* b, int64_t n_rows, int32_t ca, int32_t cb, int32_t prec,
                             const int32_t* a_amax, const int32_t* b_amax, float* scratch, float* dw, void* stream);
/* The range-grouped mode's cell limits (first position of every (offset, row range) cell in the sorted pair list) depend
 * on the map alone: gcl_conv_bwd_weight_bounds makes them once (int32[gcl_conv_bwd_weight_bounds_len(K, rows of the sorted
 * side)], 0 = the mode does not apply), gcl_conv_bwd_weight_rg takes them (`rg_bounds`, NULL = computed per launch as
 * gcl_conv_bwd_weight does).  gcl_maps_build makes them for every map with pair lists (gcl_map_desc.dw_bounds: over
 * pair_out, the sorted list of the convolution and of its transpose alike). */
int64_t gcl_conv_bwd_weight_bounds_len(int32_t K, int64_t n_sorted_rows);
int gcl_conv_bwd_weight_bounds(const int32_t* sorted_rows, const int64_t* seg_off_host, int32_t K, int64_t n_sorted_rows,
                               int32_t* bounds, void* stream);
int gcl_conv_bwd_weight_rg(const float* a, int64_t n_a, const float* b, int64_t n_b, int32_t planes, int32_t sorted_side,
                           const int32_t* pair_a, const int32_t* pair_b, const int64_t* seg_off_host, int32_t K,
                           int32_t ca, int32_t cb, int32_t prec, const int32_t* a_amax, const int32_t* b_amax,
                           float* scratch, float* dw, const int32_t* rg_bounds, void* stream);
/* What gcl_conv_bwd_weight(_rg) launches for a shape: host arithmetic, no GPU (the dispatcher itself calls the same
 * function; tests pin their cases to kernel instances with it).  planes, sorted_side as above; n_sorted_rows = rows of the
 * operand on the sorted side (n_a or n_b; any value with sorted_side 0); n_pairs_padded = seg_off_host[K].
 * out = {path (GCL_DW_PATH_*), TA, TB (channel tile of a workgroup: the template arguments; 16 x 16 for the generic
 * kernel), W (workgroups along the pair list), per (128-pair chunks per workgroup), swizzled tiles (> 0: a 1-D grid of
 * ceil(W / 8) * 8 * tiles workgroups, channel tiles of one pair range on one XCD; 0: a W x tiles grid), rr (rows per
 * range), n_ranges (range-grouped mode: a grid of ceil(n_ranges / 8) * 8 * K workgroups; else both 0)}.  The number of
 * planes of a split-precision instance follows from prec. */
#define GCL_DW_PATH_NONE 0      /* no pairs: only the reduce runs (dW = 0) */
#define GCL_DW_PATH_GENERIC 1   /* k_conv_bwd_weight_generic: channel counts that are no multiples of 32 */
#define GCL_DW_PATH_F32 2       /* k_conv_bwd_weight<TA, TB> */
#define GCL_DW_PATH_SPLIT 3     /* k_conv_bwd_weight_split<TA, TB, PL, false, false>: fp32 rows split on the fly */
#define GCL_DW_PATH_PLANES 4    /* k_conv_bwd_weight_split<TA, TB, 4, true, false>: plane images */
#define GCL_DW_PATH_RG 5        /* k_conv_bwd_weight_split<TA, TB, PL, false, true>: range-grouped */
#define GCL_DW_PATH_WG128 6     /* k_conv_bwd_weight_wg128: plane images, 128 x 128 block */
int gcl_conv_bwd_weight_launch_shape(int32_t K, int32_t ca, int32_t cb, int32_t prec, int32_t planes, int32_t sorted_side,
                                     int64_t n_sorted_rows, int64_t n_pairs_padded, int32_t out[8]);

/* First layer (Cin <= 4, Cout a multiple of 32, any ks <= 5): VALU kernels over the nbr table (one 32-column block per
 * workgroup column).  Other first-layer widths go through gcl_conv_fwd / gcl_conv_bwd_weight (generic shapes). */
/* Occupancy rows: `presence` (uint32 [n_out][ceil(K / 32)], gcl_presence_bits of `nbr`) and `not_ones` (device int32
 * [n_out], 0 = every feature row v gathers equals 1.0f; gcl_not_ones_rows) are optional and go together; cin must be 1.
 * The reference's loaders feed torch.ones((n, 1)): its test loaders and scripts for every cloud, its training loaders for
 * the neighbour clouds of a sample -- only the centre cloud carries lib/transforms.py:18 Jitter
 * (lib/colocation_data_loader.py:401-415).  For a row with flag 0, x[nbr[k][v]] is bit k of the row's presence words:
 * gcl_stem_fwd adds W[k] over the SET bits, k ascending (k_stem_fwd_occ; the table kernel is enqueued too and skips
 * those rows), gcl_stem_bwd_weight fills its 0/1 tile from the words.  Same values added in the same order: bitwise
 * identical to the table path, which every flagged row takes (flags are read on the device, no host decision).
 * gcl_not_ones_rows: a row's kernel-map neighbours share its batch index (coords[v][0], part of the key), so the flag is
 * per cloud: cloud_flags (int32 [n_cloud_flags] scratch, zeroed here) gets 1 for a batch index with a feature != 1.0f,
 * row_flags[v] = cloud_flags[batch index of v] (1 when the index does not fit the scratch). */
/* the 3^3 stride-1 kernel map of a coordinate table from its 5^3 stride-1 map (the same neighbour lookups, already
 * answered: nbr3 = 27 rows of nbr5, counts3 = their counts) -- gcl_maps_build uses it when a network asks for both
 * (conv1 5^3 + block1 3^3 on the input table, model/resunet.py:38-46, :59-60); bit-exact the direct build */
int gcl_kernel_map_3_from_5(const int32_t* nbr5, const int32_t* counts5, int64_t n, int32_t* nbr3, int32_t* counts3,
                            void* stream);
int gcl_presence_bits(const int32_t* nbr, int32_t K, int64_t n, uint32_t* bits, void* stream);
int gcl_not_ones_rows(const float* x, int32_t cin, const int32_t* coords, int64_t n, int32_t* cloud_flags,
                      int32_t n_cloud_flags, int32_t* row_flags, void* stream);
int gcl_stem_fwd(const float* x, const float* w, const int32_t* nbr, int64_t n_out, int32_t K,
                 int32_t cin, int32_t cout, float* y, const uint32_t* presence, const int32_t* not_ones, void* stream);
int64_t gcl_stem_bwd_weight_scratch_len(int32_t K, int32_t cin, int32_t cout, int64_t n_out);
int gcl_stem_bwd_weight(const float* x, const float* dy, const int32_t* nbr, int64_t n_out, int32_t K,
                        int32_t cin, int32_t cout, float* scratch, float* dw, const uint32_t* presence,
                        const int32_t* not_ones, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm over rows of [n, c] fused with the residual add and ReLU of BasicBlock.
 *   gcl_bn_stats:  mean[c], rstd[c] (biased variance, eps) and running-stat update (momentum, unbiased var).
 *                  scratch: double[gcl_bn_scratch_len(n, c)].
 *   gcl_bn_apply:  y = x * scale + shift (+ residual) (relu);   scale = w * rstd, shift = b - mean * scale.
 *                  In eval mode the host passes running stats as mean / rstd.
 *   backward:      g = dy * (relu ? y > 0 : 1);  gcl_bn_bwd_reduce -> sum_g[c], sum_gx[c] (xhat-weighted);
 *                  gcl_bn_bwd_apply -> dx, (dres = g).
 *   relu_mask (optional, uint64[gcl_bn_mask_len(n, c)]): with relu, gcl_bn_apply also writes the sign bits of y
 *                  (1 bit per element); the backward passes then take the mask instead of re-reading y (pass
 *                  y = NULL), which removes a third of their HBM traffic.
 *   y_amax / dx_amax (optional, ZERO-INITIALISED amax slots): the apply passes also publish gcl_amax of the tensor they
 *                  write, so the fp16x3 convolution that consumes it needs no extra pass over it.
 * ---------------------------------------------------------------------------------------------- */
int64_t gcl_bn_scratch_len(int64_t n, int32_t c);
int gcl_bn_stats(const float* x, int64_t n, int32_t c, float eps, float momentum,
                 float* running_mean, float* running_var, double* scratch,
                 float* mean, float* rstd, void* stream);
int64_t gcl_bn_tiles_scratch_len(int64_t n_tiles, int32_t c);   /* doubles */
int gcl_bn_stats_from_tiles(const float* partial, int64_t n_tiles, int64_t n, int32_t c, float eps, float momentum,
                            float* running_mean, float* running_var, double* scratch, float* mean, float* rstd,
                            void* stream);
int gcl_bn_apply(const float* x, int64_t n, int32_t c, const float* mean, const float* rstd,
                 const float* weight, const float* bias, const float* residual, int32_t relu,
                 float* y, uint64_t* relu_mask, int32_t* y_amax, void* stream);
/* the same with y a column slice of a wider row-major tensor (row pitch y_ld floats, 0 = c): the plan writes the decoder
 * input of an ME.cat (model/resunet.py:206,213,220) straight into the cat's output */
int gcl_bn_apply_ld(const float* x, int64_t n, int32_t c, const float* mean, const float* rstd,
                    const float* weight, const float* bias, const float* residual, int32_t relu,
                    float* y, int32_t y_ld, uint64_t* relu_mask, int32_t* y_amax, void* stream);
int64_t gcl_bn_mask_len(int64_t n, int32_t c);                  /* uint64 words */
int gcl_bn_bwd_reduce(const float* x, const float* dy, const float* y, const uint64_t* relu_mask, int64_t n,
                      int32_t c, const float* mean, const float* rstd, int32_t relu, double* scratch,
                      float* sum_g, float* sum_gx, void* stream);
/* ... with dy a column slice of a wider tensor: row pitch dy_ld floats (0 = c) */
int gcl_bn_bwd_reduce_ld(const float* x, const float* dy, int32_t dy_ld, const float* y, const uint64_t* relu_mask, int64_t n,
                         int32_t c, const float* mean, const float* rstd, int32_t relu, double* scratch, float* sum_g,
                         float* sum_gx, void* stream);
int gcl_bn_bwd_apply(const float* x, const float* dy, const float* y, const uint64_t* relu_mask, int64_t n, int32_t c,
                     const float* mean, const float* rstd, const float* weight,
                     const float* sum_g, const float* sum_gx, int32_t relu,
                     float* dx, float* dres, int32_t* dx_amax, void* stream);
int gcl_bn_bwd_apply_ld(const float* x, const float* dy, int32_t dy_ld, const float* y, const uint64_t* relu_mask, int64_t n,
                        int32_t c, const float* mean, const float* rstd, const float* weight, const float* sum_g,
                        const float* sum_gx, int32_t relu, float* dx, float* dres, int32_t* dx_amax, void* stream);

/* Round 5: plane images from the producer.  A tensor at least 128 channels wide is consumed by the fp16x3 convolutions as a
 * plane image (gcl_split_planes); the BatchNorm passes that write such a tensor write the image in the same pass, which
 * needs the tensor's power-of-two scale BEFORE the pass -- i.e. max|tensor| bounded from what is known by then:
 *   forward   gcl_bn_stats_from_tiles_range: the convolution epilogue's partials carry per-column minimum / maximum
 *             (float[4][c][n_tiles]: sum, squares, min, max); y = (x - mean) rstd w + b is monotone in x, so max|y| of a
 *             channel is attained at its minimum or maximum of x: EXACT without residual; + max|residual| (add_amax: its
 *             slot) with one; max'ed with `max_with` (the slot of the other input of an ME.cat written in place).  The
 *             bound goes to the zeroed slot y_amax, the channel ranges to xrange[2][c] (kept for the backward pass).
 *             gcl_bn_apply_planes: as gcl_bn_apply_ld; with planes != NULL it also writes the image (row pitch = y's) at
 *             the scale of y_amax's value and publishes nothing.
 *   backward  gcl_bn_bwd_reduce_range: k_bn_reduce also keeps max|g| per channel; with it, xrange and the sums,
 *             |dx| <= |w rstd| (max|g| + |sum_g| / n + max|xhat| |sum_gx| / n) goes to the zeroed slot dx_amax;
 *             gcl_bn_bwd_apply_planes writes dx's image at that scale.
 * A bound above the true maximum costs range at the bottom of the lo plane (which the range-extended format has to spare),
 * never correctness; consumers derive their scale from the same slot.
 * With planes != NULL, gcl_bn_apply_planes takes y == NULL and gcl_bn_bwd_apply_planes takes dx == NULL: the fp32 store
 * alone is skipped (nobody reads the fp32 twin), the image, the ReLU sign bits and dres are what they are with the
 * pointer given.  A NULL y / dx without planes is GCL_ERR_ARG. */
int gcl_bn_stats_from_tiles_range(const float* partial, int64_t n_tiles, int64_t n, int32_t c, float eps, float momentum,
                                  float* running_mean, float* running_var, float* mean, float* rstd, float* xrange,
                                  const float* weight, const float* bias, int32_t relu, const int32_t* add_amax,
                                  const int32_t* max_with, int32_t* y_amax, void* stream);
int gcl_bn_apply_planes(const float* x, int64_t n, int32_t c, const float* mean, const float* rstd, const float* weight,
                        const float* bias, const float* residual, int32_t relu, float* y, int32_t y_ld, uint64_t* relu_mask,
                        int32_t* y_amax, void* planes, void* stream);
int gcl_bn_bwd_reduce_range(const float* x, const float* dy, int32_t dy_ld, const float* y, const uint64_t* relu_mask,
                            int64_t n, int32_t c, const float* mean, const float* rstd, int32_t relu, double* scratch,
                            float* sum_g, float* sum_gx, const float* xrange, const float* weight, int32_t* dx_amax,
                            void* stream);
int gcl_bn_bwd_apply_planes(const float* x, const float* dy, int32_t dy_ld, const float* y, const uint64_t* relu_mask, int64_t n,
                            int32_t c, const float* mean, const float* rstd, const float* weight, const float* sum_g,
                            const float* sum_gx, int32_t relu, float* dx, float* dres, int32_t* dx_amax, void* planes,
                            void* stream);
/* The backward pair with the gradient supplied sparsely: g is the compact [cap, c] tensor (row pitch g_ld floats, 0 = c) of
 * the rows of a list (distinct rows of [0, n)); every other row of the dense dy is exactly zero.  Both entries find a row's
 * g through slots[n] (gcl_row_slots: the row's position in the list, -1 off it).
 * gcl_bn_bwd_reduce_rows reads x, g and the ReLU bits at the listed rows only and leaves what gcl_bn_bwd_reduce_range leaves,
 * bit for bit: it runs the dense pass's grid, every thread on the rows it takes there in the same order, so the fp64
 * additions are the dense pass's without its exact-zero terms -- the grid and the order depend on (n, c) only.  A padding
 * entry of the list has no slot and adds nothing.  scratch: double[gcl_bn_scratch_len(n, c)].
 * gcl_bn_bwd_apply_rows walks all n rows as gcl_bn_bwd_apply_planes does (dx is dense; a wave without a listed row loads no
 * g).  dres (optional) is COMPACT, [cap, c]: the gated gradient of the listed rows -- its padding rows are not written.
 * The ReLU gate takes the sign bits (relu_mask) only. */
int gcl_bn_bwd_reduce_rows(const float* x, const float* g, int32_t g_ld, const int32_t* slots, const uint64_t* relu_mask,
                           int64_t n, int32_t c, const float* mean, const float* rstd, int32_t relu, double* scratch,
                           float* sum_g, float* sum_gx, const float* xrange, const float* weight, int32_t* dx_amax,
                           void* stream);
int gcl_bn_bwd_apply_rows(const float* x, const float* g, int32_t g_ld, const int32_t* slots, const uint64_t* relu_mask,
                          int64_t n, int32_t c, const float* mean, const float* rstd, const float* weight, const float* sum_g,
                          const float* sum_gx, int32_t relu, float* dx, float* dres, int32_t* dx_amax, void* planes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * InstanceNorm over the rows of [n, c] (ME.MinkowskiInstanceNorm, model/common.py:7-8): every cloud of a batch is
 * normalised on its own -- per channel (x - mean) / sqrt(var + eps), biased variance over the cloud's rows -- then the
 * shared affine map, fused with the residual add and ReLU like BatchNorm.  All clouds in a fixed number of launches (four
 * per entry), rows in any order, nothing read back by the host.  Device inputs that describe the clouds:
 *   seg_off   int64 [n_clouds + 1]  prefix of the clouds' row counts (seg_off[n_clouds] = n)
 *   rows      int32 [n] or NULL     the i-th row of cloud b is rows[seg_off[b] + i]: the rows grouped by cloud, every cloud's
 *                                   rows in their order in x (a stable sort by cloud); NULL = identity (contiguous clouds)
 *   row_cloud int32 [n]             the cloud of each row
 * n_clouds (1 .. 65535) is a host integer; a cloud without rows is skipped: nothing is read or written for it, its rows of
 * the [n_clouds, c] tables keep what they held.
 * On each cloud the statistics are those of gcl_bn_stats / gcl_bn_bwd_reduce run on the cloud's rows alone, bit for bit (the
 * same chunks, threads, order of additions and conversions), and y / dx / dres those of gcl_bn_apply / gcl_bn_bwd_apply
 * with 1 / rows_b formed on the device; deterministic, no floating-point atomics.
 *   gcl_in_scratch_len(n, n_clouds, c), in doubles:
 *        (cdiv(n, 64) + n_clouds) * 2 * c      chunk sums (a chunk has at least 64 rows of one cloud)
 *      + (n_clouds + 1)                        int64 prefix of the clouds' chunk counts
 *      + (n_clouds + 1) / 2                    float 1 / rows_b per cloud
 *        0 for n <= 0, n_clouds < 1 or c < 1.
 *   gcl_in_fwd:  mean / rstd [n_clouds, c], y [n, c]; with relu the sign bits of y into relu_mask
 *                (uint64 [gcl_bn_mask_len(n, c)], ONE mask for the tensor, indexed by the tensor's own quads; required with
 *                relu); y_amax (optional, ZERO-INITIALISED amax slot) receives gcl_amax of y.
 *   gcl_in_bwd:  g = dy * (relu ? y > 0 : 1);  sum_g / sum_gx [n_clouds, c] (per cloud; the affine map's gradients are
 *                their column sums), dx [n, c], optionally dres = g and gcl_amax of dx in dx_amax.
 * c as for gcl_bn_stats (a multiple of 4 with c / 4 dividing 256); n < 2^31.
 * ---------------------------------------------------------------------------------------------- */
int64_t gcl_in_scratch_len(int64_t n, int32_t n_clouds, int32_t c);
int gcl_in_fwd(const float* x, int64_t n, int32_t c, const int64_t* seg_off, const int32_t* rows, const int32_t* row_cloud,
               int32_t n_clouds, float eps, const float* weight, const float* bias, const float* residual, int32_t relu,
               double* scratch, float* mean, float* rstd, float* y, uint64_t* relu_mask, int32_t* y_amax, void* stream);
int gcl_in_bwd(const float* x, const float* dy, int64_t n, int32_t c, const int64_t* seg_off, const int32_t* rows,
               const int32_t* row_cloud, int32_t n_clouds, const float* mean, const float* rstd, const float* weight,
               int32_t relu, const uint64_t* relu_mask, double* scratch, float* sum_g, float* sum_gx, float* dx, float* dres,
               int32_t* dx_amax, void* stream);

/* Row-wise L2 normalisation of the output features, y = x / ||x||_2 (model/resunet.py:226-230; no epsilon, as there).
 * norm[n] keeps the row norms for the backward pass: dx = (dy - y (y . dy)) / norm.  c: power of two in [4, 256].
 * dx_amax (optional, ZERO-INITIALISED amax slot): receives gcl_amax of dx (the next consumer is the `final` convolution's
 * input gradient, which needs it in the fp16x3 arithmetic). */
int gcl_row_normalize_fwd(const float* x, int64_t n, int32_t c, float* y, float* norm, void* stream);
int gcl_row_normalize_bwd(const float* y, const float* dy, const float* norm, int64_t n, int32_t c, float* dx,
                          int32_t* dx_amax, void* stream);

/* torch.optim.SGD's step (lib/colocation_trainer.py:73-77, :887: lr, momentum, weight_decay; dampening 0, no Nesterov)
 * for a list of tensors in ONE launch:  d = g + wd p;  buf = first ? d : momentum buf + d;  p -= lr buf.
 * table: DEVICE array of n_tensors x {float* p, const float* g, float* buf}; sizes: DEVICE int64[n_tensors]. */
int gcl_sgd_multi(const void* table, const int64_t* sizes, int32_t n_tensors, float lr, float momentum,
                  float weight_decay, int32_t first, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GCL loss (lib/colocation_trainer.py:430-535) and feature-space 1-NN.
 *   group g = rows index[goff[g] .. goff[g+1]) of F [n, c] (c <= 64); sel[s] = selected group ids.
 *   flags == 0 (the configuration of scripts/train_gcl_kitti.sh):
 *     pos[s]  = relu(mean_j |mean - f_j|^2 - pos_thresh)          (:474)
 *     fin[s]  = relu(|mean - f_finest|^2 - finest_thresh)         (:484-485)
 *   flags (the other config switches of the same function, and location_contrastive_loss :768-776):
 *     GCL_LOSS_SQRT   square_loss == False: distances enter as sqrt(d2 + 1e-7)                      (:470,:476,:487)
 *     GCL_LOSS_BLOCK  block_finest_gradient: mean of the NON-finest members vs the detached finest (:479-481)
 *     GCL_LOSS_PAIR   use_pair_group_positive_loss: pairpos[2 s], pairpos[2 s + 1] = the two drawn member
 *                     positions inside group sel[s]                                                  (:466-470)
 *     GCL_LOSS_NOFIN  no finest term (location_contrastive_loss)
 *   backward adds  gpos * dpos[s]/dF + gfin * dfin[s]/dF  into dF with float atomics (dF pre-zeroed by caller).
 * ---------------------------------------------------------------------------------------------- */
#define GCL_LOSS_SQRT 1
#define GCL_LOSS_BLOCK 2
#define GCL_LOSS_PAIR 4
#define GCL_LOSS_NOFIN 8
int gcl_group_loss_fwd(const float* f, int32_t c, const int64_t* index, const int64_t* goff,
                       const uint8_t* finest_flag, const int64_t* sel, int32_t n_sel,
                       float pos_thresh, float finest_thresh, int32_t flags, const int32_t* pairpos,
                       float* pos, float* fin, void* stream);
int gcl_group_loss_bwd(const float* f, int32_t c, const int64_t* index, const int64_t* goff,
                       const uint8_t* finest_flag, const int64_t* sel, int32_t n_sel,
                       float pos_thresh, float finest_thresh, int32_t flags, const int32_t* pairpos,
                       const float* gpos, const float* gfin, float* df, void* stream);
/* location_circle_loss (lib/colocation_trainer.py:538-681), per-group part: with S = log_scale (16 in the reference)
 *   pos[s] = softplus(logsumexp_i(S v_i max(v_i, 0))) / S,  v_i = dist(mean, f_i) - pos_thresh / 2      (:607-618)
 *            (GCL_LOSS_PAIR: softplus(dist(f_a, f_b) - pos_thresh), :597-605)
 *   fin[s] = the same form over v_i = dist(f_i, f_finest) - finest_thresh (GCL_LOSS_BLOCK: non-finest members only,
 *            finest detached)                                                                          (:620-640)
 *   mean_out[s][c] = the group's mean feature (:585); the negative term (:642-676) is formed by the host on the
 *   [n_sel, n_sel] matrices of these means.  max(v, 0) is a constant in the backward pass, as in the reference.
 *   backward: dF += gpos dpos/dF + gfin dfin/dF + gmean[s] / n_s (gmean may be NULL), float atomics.
 *   flags: GCL_LOSS_SQRT | GCL_LOSS_BLOCK | GCL_LOSS_PAIR. */
int gcl_circle_group_fwd(const float* f, int32_t c, const int64_t* index, const int64_t* goff,
                         const uint8_t* finest_flag, const int64_t* sel, int32_t n_sel, float pos_thresh,
                         float finest_thresh, float log_scale, int32_t flags, const int32_t* pairpos, float* pos,
                         float* fin, float* mean_out, void* stream);
int gcl_circle_group_bwd(const float* f, int32_t c, const int64_t* index, const int64_t* goff,
                         const uint8_t* finest_flag, const int64_t* sel, int32_t n_sel, float pos_thresh,
                         float finest_thresh, float log_scale, int32_t flags, const int32_t* pairpos,
                         const float* gpos, const float* gfin, const float* gmean, float* df, void* stream);

/* Row-wise nearest neighbour: for every row i of A[rows_a[i]] (rows_a may be NULL = identity) the column j
 * minimising sum_c (a - b)^2 over B[rows_b[j]]; ties -> lowest j.  dmin = that squared distance, or
 * sqrt(d2 + 1e-7) when l2 != 0 (lib/metrics.py:24-25).  The search runs as (64-row A tiles) x (chunks of B) workgroups
 * over a pair-interleaved copy of B[rows_b] made in scratch, followed by a merge over the chunks;
 * scratch: int32[gcl_nn_rowmin_scratch_len(ma, mb)], always required. */
int64_t gcl_nn_rowmin_scratch_len(int32_t ma, int32_t mb);
int gcl_nn_rowmin(const float* a, const int64_t* rows_a, int32_t ma, const float* b, const int64_t* rows_b,
                  int32_t mb, int32_t c, int32_t l2, int32_t* scratch, float* dmin, int32_t* argmin, void* stream);
/* The same search at ANY width 1 <= c <= 128 (another c is an argument error): same arguments, same difference form in
 * fp32, same tie rule, same l2.  The channels are zero-padded to the next multiple of 8 in the interleaved copy and in the
 * A registers (a padded channel adds fma(0, 0, acc): exact).  Summation order: one chain per (row, column) over ascending
 * channels, d2 = (a_0 - b_0)^2 rounded, then d2 = fma(a_k - b_k, a_k - b_k, d2), k = 1 .. c - 1 -- at c = 16 / 32 / 64 the
 * order of gcl_nn_rowmin, bit for bit; that entry stays the one for those widths (lib/metrics.py::pdist_min dispatches;
 * it is ~12 % faster at 32 channels).  A thread keeps its A row as single floats, which is what lets 128 channels fit
 * (csrc/loss.hip, k_nn_rowmin_any).
 * scratch: int32[gcl_nn_rowmin_any_scratch_len(ma, mb, c)], always required (0 for empty input or c out of range). */
int64_t gcl_nn_rowmin_any_scratch_len(int32_t ma, int32_t mb, int32_t c);
int gcl_nn_rowmin_any(const float* a, const int64_t* rows_a, int32_t ma, const float* b, const int64_t* rows_b,
                      int32_t mb, int32_t c, int32_t l2, int32_t* scratch, float* dmin, int32_t* argmin, void* stream);
/* A BATCH of such searches in the launches of one: one interleave launch, one search launch with the search as the grid's
 * z dimension, and one merge launch when some search runs in more than one chunk -- whatever n_searches is.  Widths 16 /
 * 32 / 64 run the chain of gcl_nn_rowmin, every other width in 1 .. 128 that of gcl_nn_rowmin_any (the same device
 * functions), and the minimum is exact with ties to the lowest index under any chunking: dmin / argmin of a search are bit
 * for bit those of the single entry, alone, at any position of any batch, on every run.  Ragged: every search has its own
 * ma / mb / row lists; searches may share a, b or both (the two directions of a pair).  c and l2 are per call.
 * Optional fused gather, per search: with pts_a and pts_b (float [*, 3]; both or neither) the kernel that writes argmin[r]
 * also writes  src[r] = pts_a[rows_a ? rows_a[r] : r]  and  tgt[r] = pts_b[rows_b ? rows_b[argmin[r]] : argmin[r]]
 * (float [ma, 3] each; they may be slices of a batch's padded correspondence buffers).
 * The table is passed TWICE: searches_host, from which the entry validates and sizes grids and chunks, and searches (a
 * device copy of the same bytes) for the kernels; the entry allocates, copies and synchronises nothing.
 * gcl_nn_rowmin_batch_scratch_len FILLS bi_off / part_off of every record (offsets into scratch, in 32-bit words) and
 * returns the scratch length in words: call it on the host table before copying the table to the device.  It returns 0
 * for n_searches < 1, c outside 1 .. 128 or an empty search.  Per search: the interleaved copy of B (cdiv(mb, 2) * 2 * cp
 * words, cp = c rounded up to 8; 64 for c = 16 / 32 as the single entry sizes it) plus, when it runs in several chunks,
 * 2 * n_chunks * ma words; the chunk size aims at ~1536 workgroups for the whole batch. */
typedef struct gcl_nn_search {
  const float* a;             /* float [*, c] */
  const int64_t* rows_a;      /* int64 [ma] or NULL = rows 0 .. ma - 1 */
  const float* b;
  const int64_t* rows_b;      /* int64 [mb] or NULL */
  float* dmin;                /* float [ma] */
  int32_t* argmin;            /* int32 [ma] */
  const float* pts_a;         /* optional gather (both or neither) */
  const float* pts_b;
  float* src;                 /* float [ma, 3], required with pts_a / pts_b */
  float* tgt;
  int64_t bi_off, part_off;   /* filled by gcl_nn_rowmin_batch_scratch_len */
  int32_t ma, mb;
} gcl_nn_search;
int64_t gcl_nn_rowmin_batch_scratch_len(gcl_nn_search* searches_host, int32_t n_searches, int32_t c);
int gcl_nn_rowmin_batch(const gcl_nn_search* searches_host, const gcl_nn_search* searches, int32_t n_searches, int32_t c,
                        int32_t l2, int32_t* scratch, void* stream);

/* 3-D nearest point (generalization_ETH/evaluate.py:110-122, find_nearest_voxel_feature): for every query q[i]
 * (float [m, 3]) the row j of p (float [n, 3]) that minimises (qx - px)^2 + (qy - py)^2 + (qz - pz)^2, evaluated in that
 * DIFFERENCE form in fp32 (never |q|^2 + |p|^2 - 2 q.p, which loses 5 cm voxels at outdoor coordinates); exact search,
 * ties -> lowest j.  argmin int32 [m]; d2min float [m] (the squared distance) may be NULL.  When feat (float [n, c], any
 * c >= 1) and desc (float [m, c]) are given -- both or neither -- the same call writes desc[i] = feat[argmin[i]].
 * Runs as (256-query tiles) x (chunks of p) workgroups, then a merge over the chunks when there are several;
 * scratch: int32[gcl_nn3_scratch_len(m, n)] (0 for a single chunk: scratch may then be NULL).
 * m == 0 returns 0 without a launch; n <= 0 is an argument error. */
int64_t gcl_nn3_scratch_len(int32_t m, int32_t n);
int gcl_nn3_rowmin(const float* q, int32_t m, const float* p, int32_t n, const float* feat, int32_t c, int32_t* scratch,
                   float* d2min, int32_t* argmin, float* desc, void* stream);
/* Mutual filter and inlier count of one fragment pair (generalization_ETH/evaluate.py:63-77 calculate_M, :160-169):
 * nn01 int32 [m0] = nearest target of every source, nn10 int32 [m1] = nearest source of every target.  pairs
 * (int32 [m0, 2]) receives every (i, nn01[i]) with nn10[nn01[i]] == i, densely packed in ascending i (the same list
 * on every run; rows from stats[0] on are left as they were); an entry of nn01 outside [0, m1) is not mutual and is never
 * dereferenced.  stats int32 [2]: [0] = number of mutual pairs, [1] = how many of them have
 * |kp0[i] - (R kp1[j] + t)| < tau when T (float [12] on the device, row-major [R | t]) is given -- kp0 float [m0, 3] and
 * kp1 float [m1, 3] are then required; the TARGET keypoints are moved, as the reference does with gtTrans -- else 0.
 * `stats` is any int32 pair of the caller's: the pairs of a scene fill one [P, 2] table that is read once.
 * m0 == 0 writes stats = {0, 0}. */
int gcl_mutual_match(const int32_t* nn01, int32_t m0, const int32_t* nn10, int32_t m1, const float* kp0, const float* kp1,
                     const float* T, float tau, int32_t* pairs, int32_t* stats, void* stream);
/* The correspondences of a registration under open3d's mutual filter (registration_ransac_based_on_feature_matching with
 * mutual_filter = true), as point rows, their number left on the device.  nn01 / nn10 as gcl_mutual_match takes them (an
 * entry outside the range is never mutual and never dereferenced), xyz0 float [m0, 3], xyz1 float [m1, 3].  Let M be the
 * pairs (i, nn01[i]) with nn10[nn01[i]] == i in ascending i.  |M| >= min_count: row k of src / tgt (float [m0, 3]) is
 * xyz0[i_k] / xyz1[j_k], rows from |M| on are zero, count (int32 [2]) = {|M|, |M|}.  Otherwise open3d's fall-back to the
 * original correspondences: row i is xyz0[i] / xyz1[nn01[i]] (a zero target row where nn01[i] is out of range) and
 * count = {m0, |M|}.  count[0] is what gcl_ransac_register_batch takes as a pair's n_dev entry, and src / tgt / count may be
 * slices of a batch's buffers: nothing is read back.  Ordered compaction by one workgroup: the same list on every run. */
int gcl_mutual_correspondences(const int32_t* nn01, int32_t m0, const int32_t* nn10, int32_t m1, const float* xyz0,
                               const float* xyz1, int32_t min_count, float* src, float* tgt, int32_t* count, void* stream);
/* Both filters for a BATCH of pairs in one launch, one workgroup per pair (the single entries run one workgroup and leave
 * the other CUs idle: eight pairs are eight such launches in a row).  The kernel bodies are those of the single entries, so
 * a pair's outputs are bit for bit theirs.  jobs_host / jobs: the table on the host (validated) and its device copy (read
 * by the kernel).  gcl_mutual_match_batch reads nn01, m0, nn10, m1, xyz0 (= kp0), xyz1 (= kp1), T and writes pairs and
 * count (= stats); gcl_mutual_correspondences_batch reads nn01, m0, nn10, m1, xyz0, xyz1 and writes src, tgt, count.  tau
 * and min_count are per call. */
typedef struct gcl_mutual_job {
  const int32_t* nn01;
  const int32_t* nn10;
  const float* xyz0;
  const float* xyz1;
  const float* T;             /* float [12] or NULL (gcl_mutual_match_batch) */
  int32_t* pairs;             /* int32 [m0, 2] (gcl_mutual_match_batch) */
  float* src;                 /* float [m0, 3] (gcl_mutual_correspondences_batch) */
  float* tgt;
  int32_t* count;             /* int32 [2]: stats / count of the single entries */
  int32_t m0, m1;
} gcl_mutual_job;
int gcl_mutual_match_batch(const gcl_mutual_job* jobs_host, const gcl_mutual_job* jobs, int32_t n_pairs, float tau,
                           void* stream);
int gcl_mutual_correspondences_batch(const gcl_mutual_job* jobs_host, const gcl_mutual_job* jobs, int32_t n_pairs,
                                     int32_t min_count, void* stream);

/* keep[r] = (sel1[r] != sel2[arg[r]]) && the pair {sel1[r], sel2[arg[r]]} shares no positive group
 * (equivalent to the reference's `~np.isin(_neg_hash(...), index_hash)` :521-529: the symmetric key is
 * collision-free).  table: int64[cap,2] scratch hash table (cap = pow2 >= 2*m). */
int gcl_neg_mask(const int64_t* sel1, const int64_t* sel2, const int32_t* arg, int32_t m,
                 const int64_t* index, const int64_t* goff, int64_t n_groups, int64_t n_index,
                 int64_t* table, int64_t cap, uint8_t* keep, void* stream);
/* neg = mean over kept rows of relu(thresh - dmin)^2 (NaN when nothing is kept, as torch's mean of empty);
 * out[0] = neg, out[1] = #kept.  Backward scatters into dF (atomics). */
int gcl_neg_loss_fwd(const float* dmin, const uint8_t* keep, int32_t m, float thresh, float* out, void* stream);
int gcl_neg_loss_bwd(const float* f, int32_t c, const int64_t* sel1, const int64_t* sel2, const int32_t* arg,
                     const float* dmin, const uint8_t* keep, int32_t m, float thresh, const float* out,
                     const float* gneg, float* df, void* stream);
/* The step's scalar arithmetic in one launch each way (lib/colocation_trainer.py:533-535, :865-868):
 * out = {total, pos_mean, fin_mean, neg} with pos_mean = sum(pos) / n_sel, fin_mean = sum(fin) / n_sel,
 * total = w_pos * pos_mean + w_fin * fin_mean + w_neg * neg[0]; gcl_loss_seed writes the upstream gradients of the
 * terms for gcl_group_loss_bwd / gcl_neg_loss_bwd from the gradient of the total: gpos[i] = gfin-alike
 * (g * w) / n_sel, gneg[0] = g * w_neg. */
int gcl_loss_combine(const float* pos, const float* fin, int32_t n_sel, const float* neg, float w_pos, float w_fin,
                     float w_neg, float* out, void* stream);
int gcl_loss_seed(const float* g_total, float w_pos, float w_fin, float w_neg, int32_t n_sel, float* gpos, float* gfin,
                  float* gneg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SC2-PCR registration back-end (scripts/SC2_PCR/SC2_PCR.py, Matcher.SC2_PCR :304-381) for ONE pair:
 * src / tgt float [n, 3] = the putative correspondences (n <= 8192).  No [n, n] matrix is materialised; ties of the
 * reference's argsort / argmax go to the lowest index.  Call order (the host keeps the few glue steps):
 *   gcl_sc2_confidence  leading eigenvector of the first-order compatibility matrix by power iteration with the
 *                       reference's torch.allclose early stop (:337-345, :167-185).  x float[n] must hold ones,
 *                       done int32[1] zero; partial float[gcl_sc2_chunks() * n].  Result in x.
 *   gcl_sc2_local_max   non-maximum suppression flags (:43-47); is_max int32[n] must hold ones.
 *                       host: seeds = first int(n * ratio) of a stable descending sort of conf * is_max.
 *   gcl_sc2_seed_knn    tight-compatibility bit matrix (bits uint64[n * ceil(n / 64)]), second-order measure of every
 *                       seed and its k1 (<= 32) best correspondences, knn int32[n_seeds * k1] (:353-361, :85-86).
 *   gcl_sc2_seed_trans  per seed: k2-subset by the local second-order measure, k2 x k2 power iteration
 *                       (num_iterations steps), weighted Kabsch -> trans float[n_seeds * 12] (rows of [R | t]);
 *                       fitness float[n_seeds] = inlier count under inlier_thresh (:88-161).
 *                       host: best = lowest index of the maximum fitness.
 *   gcl_sc2_refine      post refinement in place on T float[12] (:238-279): up to `iterations` weighted Kabsch steps
 *                       over the inliers under thr, stopping when the inlier count repeats.
 *                       One launch.  state int32[2]; partial double[gcl_sc2_refine_partial_len()] is UNUSED (the scratch
 *                       of an earlier two-kernel form: kept in the signature, must not be null).
 * ---------------------------------------------------------------------------------------------- */
int32_t gcl_sc2_chunks(void);
int32_t gcl_sc2_refine_partial_len(void);
int gcl_sc2_confidence(const float* src, const float* tgt, int32_t n, float d_thre, int32_t num_iterations,
                       float* partial, float* x, int32_t* done, void* stream);
/* the same power iteration over the NON-ZERO entries of the compatibility matrix, kept from ONE build pass per registration
 * in an ELL layout (every (row, column chunk) segment has its own place of chunk-length entries; scratch:
 * gcl_sc2_confidence_scratch_bytes(n) bytes = n^2 entries of address space, 512 MB at n = 8000, of which only the non-zero
 * ones are touched): the same non-zero terms in the same order, i.e. bitwise the result x of gcl_sc2_confidence, without
 * re-deriving 64 M entries (two square roots each) in every one of the 20 products.  `partial` is working space here (the
 * products alternate between it and a second buffer in scratch: product k normalises product k - 1 itself, 21 launches
 * instead of 40) */
int64_t gcl_sc2_confidence_scratch_bytes(int32_t n);
int gcl_sc2_confidence_sparse(const float* src, const float* tgt, int32_t n, float d_thre, int32_t num_iterations,
                              float* partial, float* x, int32_t* done, void* scratch, void* stream);
/* One call per registration (round 5): Matcher.SC2_PCR + the labels of Matcher.estimator (:304-381, :404-409) as ONE launch
 * sequence -- gcl_sc2_confidence_sparse, gcl_sc2_local_max, the seed order (stable argsort of -(conf * is_max): value
 * descending, index ascending), gcl_sc2_seed_knn, gcl_sc2_seed_trans, the best seed (lowest index of the maximum fitness),
 * gcl_sc2_refine, and the [4, 4] result with labels[i] = |R s_i + t - t'_i| < inlier_thresh -- without the host in between
 * (the Python Matcher issued ~25 torch operations and 7 calls per pair: 1 ms of host time in a loop that is host-bound).
 * Outputs: conf float[n], seeds int64[n_seeds], knn int32[n_seeds * k1], seed_trans float[n_seeds * 12],
 * fitness float[n_seeds], best int32[1], trans16 float[16] (row-major [4, 4]), labels float[n] (0 / 1).
 * scratch: gcl_sc2_register_scratch_bytes(n) bytes.  FOOTPRINT: ~ 8 n^2 bytes of ADDRESS SPACE -- 528 MB at n = 8000 -- for the
 * confidence's kept non-zero entries (an ELL slab: n^2 (column, value) places of 8 bytes, of which only the non-zero entries
 * are ever touched, i.e. only those cost bandwidth or physical pages' worth of traffic) + the 8 MB tight-compatibility bit
 * matrix; the seed stage's uint16 second-order rows (2 n_seeds n bytes) reuse the slab once the last product has run.  That
 * is two of the four dense [n, n] float matrices the reference allocates (scripts/SC2_PCR/SC2_PCR.py:327-361); with several
 * registrations in flight (GCL_EVAL_STREAMS > 1) every one needs its own block.  Same results as the staged calls.
 * The launches are those of gcl_sc2_register_batch for one pair, with plain arguments, on one slot of its scratch layout:
 * gcl_sc2_register_scratch_bytes(n) = gcl_sc2_register_batch_scratch_bytes(1, n).  num_iterations = 0: no products, conf stays
 * at ones (the build pass still runs: it makes the tight compatibility bits). */
int64_t gcl_sc2_register_scratch_bytes(int32_t n);
int gcl_sc2_register(const float* src, const float* tgt, int32_t n, float d_thre, int32_t num_iterations, float nms_radius,
                     int32_t n_seeds, int32_t k1, int32_t k2, float inlier_thresh, float refine_thr, int32_t refine_iters,
                     void* scratch, float* conf, int64_t* seeds, int32_t* knn, float* seed_trans, float* fitness,
                     int32_t* best, float* trans16, float* labels, void* stream);
/* A BATCH of pairs in the launches of ONE registration (the reference asserts bs == 1; its Matcher is written for
 * [bs, num_corr, 3]).  src / tgt: [batch, n_cap, 3] on the device; pair b uses rows 0 .. counts[b] - 1 of its block and
 * wants n_seeds[b] seeds.  counts / n_seeds are HOST arrays [batch]: they travel to the kernels as a by-value argument (no
 * copy on the stream, no read-back, no synchronisation).  Every launch of a registration is made once, with
 * the pair as the grid's z dimension and grids sized for n_cap and S = max(n_seeds); a workgroup reads its own pair's n,
 * derives that pair's chunk length, word count and tile counts, and returns at once when it lies beyond them.  The early
 * exits (the power iteration's `done`, the refinement's convergence) are per pair.  More than 32 pairs: one such launch
 * sequence per 32.
 * CONTRACT: for every pair, every output is bit for bit what gcl_sc2_register writes for that pair alone, whatever the
 * other pairs of the batch are and in whatever order: the two entries launch the same stage bodies, and a body's sums of
 * products are written out operation by operation, so its bits do not depend on the kernel it is compiled into.
 * num_iterations = 0 as in the single call.
 * Outputs: trans16 float[batch, 16], labels float[batch, n_cap] (0 from a pair's count on), conf float[batch, n_cap],
 * seeds int64[batch, S], knn int32[batch, S, k1], seed_trans float[batch, S, 12], fitness float[batch, S], best int32[batch];
 * entries beyond a pair's own extent are unspecified, except labels.
 * Needs 1 <= n_seeds[b] <= counts[b] <= n_cap <= 8192, batch >= 1, k1 <= min(counts), no null pointer: checked before any
 * GPU call (GCL_ERR_ARG, gcl_last_error).
 * scratch: gcl_sc2_register_batch_scratch_bytes(batch, n_cap) bytes = batch slots sized for n_cap, every
 * slot and every slab in it on a 256-byte boundary (0 for batch <= 0, n_cap <= 0 or n_cap > 8192); may hold anything, the call
 * initialises what it reads.  SCRATCH FOOTPRINT: ~ 8 n_cap^2 bytes of address space PER PAIR -- 528 MB at n = 8000, 4.2 GB for
 * 8 such pairs -- of which, as in the single call, only the non-zero entries are ever touched. */
int64_t gcl_sc2_register_batch_scratch_bytes(int32_t batch, int32_t n_cap);
int gcl_sc2_register_batch(const float* src, const float* tgt, int32_t batch, int32_t n_cap, const int32_t* counts,
                           const int32_t* n_seeds, float d_thre, int32_t num_iterations, float nms_radius, int32_t k1,
                           int32_t k2, float inlier_thresh, float refine_thr, int32_t refine_iters, void* scratch, float* conf,
                           int64_t* seeds, int32_t* knn, float* seed_trans, float* fitness, int32_t* best, float* trans16,
                           float* labels, void* stream);
int gcl_sc2_local_max(const float* src, const float* conf, int32_t n, float radius, int32_t* is_max, void* stream);
int gcl_sc2_seed_knn(const float* src, const float* tgt, int32_t n, const int64_t* seeds, int32_t n_seeds,
                     float d_thre, int32_t k1, uint64_t* bits, int32_t* knn, void* stream);
int gcl_sc2_seed_trans(const float* src, const float* tgt, int32_t n, const int32_t* knn, int32_t n_seeds, int32_t k1,
                       int32_t k2, float d_thre, int32_t num_iterations, float inlier_thresh, float* trans,
                       float* fitness, void* stream);
int gcl_sc2_refine(const float* src, const float* tgt, int32_t n, float thr, int32_t iterations, double* partial,
                   int32_t* state, float* T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Feature-matching RANSAC registration for ONE pair (open3d's registration_ransac_based_on_feature_matching on the
 * correspondences src[i] <-> tgt[i], float [n, 3]; callers scripts/test_kitti.py:171-178 -- ransac_n 4, edge-length
 * checker 0.9, distance checker and inlier distance one voxel, 4 000 000 iterations -- and
 * generalization_ETH/evaluate.py:171-186 -- ransac_n 3, 0.05, 50 000).  One call enqueues everything; nothing is read back.
 * Hypothesis h in [0, max_iteration) is a function of (seed, h) alone (a counter generator in place of open3d's
 * std::mt19937; csrc/ransac.hip states the draw), so equal inputs give bitwise equal outputs:
 *   draw ransac_n indices (repeated index: status -3)  ->  CorrespondenceCheckerBasedOnEdgeLength(edge_similarity) on the
 *   sample (-1; <= 0: off)  ->  TransformationEstimationPointToPoint(false) on the sample, fp64 Kabsch, fp32 [R | t]  ->
 *   CorrespondenceCheckerBasedOnDistance(check_distance) on the sample (-2; <= 0: off)  ->  inlier count (|R s + t - t'| <
 *   max_corr_distance, fp32) and sum of squared inlier distances over all n (status = count).
 * Winner: highest count, then lower sum (IsBetterRANSACThan), then lower h.  Hypotheses are processed in chunks of `chunk`
 * consecutive ids (0 = gcl_ransac_default_chunk(); values above 2^20 are taken as 2^20); after each chunk, with
 * 0 < confidence < 1, limit = ceil(log(1 - confidence) / log(1 - (best count / n)^ransac_n)) and a later chunk whose first
 * id is >= limit does nothing (its hypotheses: status -4) -- a word on the device, no host round trip.  With the stop off
 * (confidence outside (0, 1)) the result does not depend on `chunk`.
 * Outputs: trans16 float[16] (row-major [4, 4]); info int32[4] = {winning h or -1, its inlier count, hypotheses covered by
 * executed chunks, hypotheses scored}; fit float[2] = {count / n, sqrt(sum / count)}; labels float[n] (optional): 1 for the
 * winner's inliers; hyp_status int32[max_iteration] (optional): the status above, a diagnostic and test hook.  Nothing scored
 * or best count 0: identity, info[0] = -1, fit = {0, 0}.  scratch: gcl_ransac_scratch_bytes(n, chunk) bytes (ransac_n <= n <= 2^24).
 * ---------------------------------------------------------------------------------------------- */
int64_t gcl_ransac_scratch_bytes(int32_t n, int32_t chunk);
int32_t gcl_ransac_default_chunk(void);
int gcl_ransac_register(const float* src, const float* tgt, int32_t n, int32_t ransac_n, float edge_similarity,
                        float check_distance, float max_corr_distance, int32_t max_iteration, float confidence,
                        uint64_t seed, int32_t chunk, void* scratch, float* trans16, int32_t* info, float* fit,
                        float* labels, int32_t* hyp_status, void* stream);
/* The same registration for a BATCH of pairs in the launches of one: src / tgt float [batch, n_cap, 3], every kernel takes
 * the pair as a grid dimension, the chunk loop is enqueued once for all pairs.  Pair b runs on its first n_b correspondences,
 * n_b = n_dev[b] read ON THE DEVICE (device int32 [batch]; a negative value reads as 0, one above n_cap as n_cap; NULL: n_cap
 * for every pair) -- the host never knows it, so it may be the count gcl_mutual_correspondences has just written.  Rows at or
 * beyond n_b are never read.  seeds is a HOST array [batch] (copied into the launch arguments).  Outputs per pair:
 * trans16 [batch, 16], info [batch, 4], fit [batch, 2] (count / n_b), labels [batch, n_cap] (optional; 0 from n_b on),
 * hyp_status [batch, max_iteration] (optional).  For n_b >= ransac_n every output of pair b is bitwise what
 * gcl_ransac_register gives for those n_b correspondences and seeds[b], whatever else is in the batch and whatever n_cap is
 * (gcl_ransac_register IS a batch of one).  The confidence stop is per pair: a pair past its own limit does nothing in later
 * chunks (status -4) while the others go on.  n_b < ransac_n (possible only with n_dev): nothing is drawn; identity,
 * info = {-1, 0, 0, 0}, fit = {0, 0}, labels 0, every status -4.
 * SCRATCH FOOTPRINT: gcl_ransac_batch_scratch_bytes(batch, n_cap, chunk) = batch x gcl_ransac_scratch_bytes(n_cap, chunk):
 * every pair has its own control block and its own slice of the single-pair layout, ~ 150 bytes per hypothesis of a chunk,
 * i.e. about 40 MB PER PAIR at the default chunk of 262 144 (320 MB for 8 pairs); a smaller chunk shrinks it in proportion.
 * 1 <= batch <= 65535, ransac_n <= n_cap <= 2^24; the query returns 0 for arguments outside these ranges. */
int64_t gcl_ransac_batch_scratch_bytes(int32_t batch, int32_t n_cap, int32_t chunk);
int gcl_ransac_register_batch(const float* src, const float* tgt, int32_t batch, int32_t n_cap, const int32_t* n_dev,
                              int32_t ransac_n, float edge_similarity, float check_distance, float max_corr_distance,
                              int32_t max_iteration, float confidence, const uint64_t* seeds, int32_t chunk, void* scratch,
                              float* trans16, int32_t* info, float* fit, float* labels, int32_t* hyp_status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Registration statistics of a BATCH of pairs in one launch: the scoring of the reference's SC2-PCR benchmark loops
 * (scripts/SC2_PCR/test_KITTI.py:46-69, test_3DMatch.py:46-73; evaluate_metric.py TransformationLoss / ClassificationLoss).
 * src_corr / tgt_corr float [batch, n_cap, 3]; pair b has n_b = counts[b] correspondences, read ON THE DEVICE (device int32
 * [batch], clamped to [0, n_cap]; NULL: n_cap for every pair; the convention of gcl_ransac_register_batch's n_dev) -- rows
 * at or beyond n_b are never read.  pred_trans / gt_trans float [batch, 16] (row-major [4, 4]).  re_thre in degrees,
 * te_thre in centimetres.  stats double [batch, 10]:
 *   0 success (RE < re_thre and TE < te_thre)      1 RE (deg) = acos(clamp((trace(R^T R_gt) - 1) / 2, -1, 1)) 180 / pi
 *   2 TE (cm) = 100 |t - t_gt|                      3 #gt inliers: |R_gt p + t_gt - q| < inlier_threshold, the distance
 *   4 column 3 / n_b                                  in fp32 as sum(d^2) ** 0.5
 *   5 #gt inliers among the predicted inliers (the same expression under pred_trans)
 *   6 precision = col 5 / #predicted   7 recall = col 5 / col 3   8 F1 = 2 col 5 / (#predicted + col 3)   (0 / 0 -> 0)
 *   9 mean over the pair of |R p + t - q| under pred_trans (TransformationLoss's RMSE), in fp64
 * RE, TE and the ratios are formed in fp64 from the fp32 matrices and the integer counts; n_b = 0 gives 0 in columns 3 - 9.
 * pred_labels / gt_labels float [batch, n_cap] (each optional): the two labels, 0 from n_b on.
 * One workgroup per pair, fixed-order reduction: the same table on every run.  batch == 0 returns 0 without a launch.
 * ---------------------------------------------------------------------------------------------- */
int gcl_registration_stats(const float* src_corr, const float* tgt_corr, int32_t batch, int32_t n_cap, const int32_t* counts,
                           const float* pred_trans, const float* gt_trans, float inlier_threshold, float re_thre,
                           float te_thre, double* stats, float* pred_labels, float* gt_labels, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Native step runtime (round 3): ONE call enqueues a whole pass.
 *
 * The per-operator entries above are what ME's operator surface binds; a training step calls ~560 of them, and from
 * Python each costs ~40 us of interpreter + ctypes time -- the step was bound by the host.  The two families below issue
 * the same launches, with the same arguments and in the same order, from C:
 *   gcl_maps_*  everything CoordinateManager builds for a network (lib/colocation_trainer.py:843-845 -> ME's
 *               coordinate manager: stride maps, kernel maps, mask-sorted tables, pair lists) in one call;
 *   gcl_plan_*  the forward / backward pass of a network described as a list of operator records (what
 *               model/resunet.py:173-232 and model/residual_block.py:37-53 call on the ME surface).
 * Results are bitwise identical to the per-operator path (tests/test_gpu_plan.py).
 * Memory stays with the caller: both families carve every tensor they need from an ARENA the caller passes (a device
 * buffer; size from gcl_maps_arena_bytes / gcl_plan_arena_bytes); plan handles own host memory only.
 * ---------------------------------------------------------------------------------------------- */
#define GCL_MAX_LEVELS 8
#define GCL_MAX_MAPS 16
#define GCL_ERR_ARENA (-4)     /* the arena is too small */
#define GCL_MAPS_PINNED_BYTES (512 * (GCL_MAX_MAPS + 1))

/* one kernel map to build: CoordinateManager.get_kernel_map(t_in, kernel_size, stride);
 * tables bit 0 / bit 1: gcl_table_sort of nbr / of nbr_t; bit 2: presence words of nbr (the Cin <= 4 first layer's
 * occupancy path); pairs != 0: the weight gradient's pair lists.
 * kernel_size 1 (stride 1): only the identity pair list of level t_in (pairs != 0). */
typedef struct gcl_map_spec {
  int32_t t_in, kernel_size, stride, tables, pairs;
} gcl_map_spec;

/* one kernel map as built; pointers are DEVICE pointers into the arena (NULL = not requested), seg_off HOST values */
typedef struct gcl_map_desc {
  int32_t t_in, kernel_size, stride, K;
  int32_t level_in, level_out;          /* indices into gcl_maps_desc.n_rows (level i = tensor stride 2^i) */
  int64_t n_in, n_out, n_pairs;
  int32_t *nbr, *nbr_t, *counts;
  int32_t *tbl_n, *order_n, *mask_n;    /* gcl_table_sort(nbr) */
  int32_t *tbl_t, *order_t, *mask_t;    /* gcl_table_sort(nbr_t) */
  int32_t *pair_in, *pair_out;
  uint32_t* presence;                   /* gcl_presence_bits(nbr) when the spec asks for it (tables bit 2), else NULL */
  int32_t* dw_bounds;                   /* gcl_conv_bwd_weight_bounds over pair_out (maps with pair lists and >= 32768 out rows), else NULL */
  int64_t seg_off[128];                 /* padded prefix sums of the per-offset pair counts, K + 1 used */
  int32_t counts_host[128];
} gcl_map_desc;

typedef struct gcl_maps_desc {
  int32_t n_levels, n_maps;
  int64_t n_rows[GCL_MAX_LEVELS];
  int32_t* coords[GCL_MAX_LEVELS];      /* int32 [n_rows, 4] */
  int64_t* table[GCL_MAX_LEVELS];       /* coordinate hash table of the level, int64 [cap, 2] */
  int64_t cap[GCL_MAX_LEVELS];
  int32_t status[4];                    /* HOST copy of gcl_coords_insert's status words */
  int64_t arena_used;
  void* ready_event;                    /* split build: hipEvent_t the CALLER records on the side stream after the call (else NULL) */
  int32_t late_mask;                    /* split build: bit s = map s was enqueued on the side stream (gcl_maps_build_split) */
  int32_t reserved;
  gcl_map_desc maps[GCL_MAX_MAPS];
} gcl_maps_desc;

/* Upper bound of the arena gcl_maps_build needs for n stride-1 rows. */
int64_t gcl_maps_arena_bytes(int64_t n, const gcl_map_spec* specs_host, int32_t n_specs, int32_t n_levels);
/* Builds levels 0 .. n_levels-1 (tensor strides 1, 2, 4, ...) from `coords` (int32 [n,4], device) and every map of
 * `specs_host`, with exactly the launches of the per-operator entries.  SYNCHRONISES `stream` twice (level sizes, pair
 * counts) -- call it from a loader-side thread on a side stream.  pinned_host: >= GCL_MAPS_PINNED_BYTES of page-locked HOST
 * memory used for the two read-backs.  Fills *out_host; returns GCL_ERR_ARG for duplicate / out-of-range coordinates
 * (out_host->status tells which). */
int gcl_maps_build(const int32_t* coords, int64_t n, const gcl_map_spec* specs_host, int32_t n_specs, int32_t n_levels,
                   void* arena, int64_t arena_bytes, void* pinned_host, gcl_maps_desc* out_host, void* stream);
/* The same build on TWO streams, for a pass over few rows (one pair of clouds per call: util/misc.py:128-130,
 * scripts/test_kitti.py:143-150), whose ~ 90 small dependent launches are a third of the pass.  Everything up to the read-back
 * of the level sizes runs on `stream`; after it -- when no map asks for pair lists, i.e. nothing else waits for the host --
 * the maps of the input level alone (kernel maps with t_in = 1, stride 1: what a network's first layers use) and their sorted
 * tables stay on `stream`, every other map goes to `side_stream` (out_host->late_mask).  The caller records an event on
 * side_stream after the call and stores it in out_host->ready_event: gcl_plan_forward / _eval make `stream` wait for it in
 * front of the first record that uses a late map, so the first layers' convolutions run beside the deeper levels' map
 * building.  Same launches, same results as gcl_maps_build (side_stream NULL, or pair lists wanted: exactly that call). */
int gcl_maps_build_split(const int32_t* coords, int64_t n, const gcl_map_spec* specs_host, int32_t n_specs, int32_t n_levels,
                         void* arena, int64_t arena_bytes, void* pinned_host, gcl_maps_desc* out_host, void* stream,
                         void* side_stream);

/* Operator records of a network pass.  Tensors are numbered 0 .. n_tensors-1 (0 = the input features); every record
 * names its input(s) and its output; parameters are numbered in the order of the `params` / `grads` pointer arrays. */
#define GCL_OP_CONVBN 1    /* y = BatchNorm(conv(x)) (+ residual x2) (relu): MinkowskiConvolution(+Transpose) + MinkowskiBatchNorm */
#define GCL_OP_CONV 2      /* y = conv(x) (+ bias) */
#define GCL_OP_RELU 3      /* MEF.relu */
#define GCL_OP_CAT 4       /* ME.cat(x, x2) */
#define GCL_OP_ROWNORM 5   /* y = x / ||x||_2 per row (model/resunet.py:226-230) */
typedef struct gcl_plan_op {
  int32_t kind;
  int32_t x, x2, y;          /* tensor ids; x2 = residual (CONVBN) / second input (CAT), -1 = none */
  int32_t level_in, level_out, cin, cout;
  int32_t map, transpose, K; /* map = index into gcl_maps_desc.maps (kernel_size 1: the identity-pair entry) */
  int32_t w, bias;           /* parameter ids: kernel [K, cin, cout], bias [1, cout] or -1 */
  int32_t bn_w, bn_b, bn;    /* parameter ids of the BatchNorm affine pair; bn = index of its running-statistics pair */
  int32_t relu;
  float momentum, eps;
} gcl_plan_op;

/* Plan handle: host memory only.  weight_order[n_weights] = parameter ids of the MFMA-shaped convolution kernels in
 * the order their max-abs slots / packed images are laid out (WeightAmaxGroup).  NULL on error (gcl_last_error). */
void* gcl_plan_create(const gcl_plan_op* ops_host, int32_t n_ops, int32_t n_tensors, int32_t n_params,
                      const int32_t* weight_order_host, int32_t n_weights, int32_t presplit_min_c);
void gcl_plan_destroy(void* plan);
/* persistent DEVICE state the caller keeps for a plan (pointer / descriptor tables), bytes */
int64_t gcl_plan_state_bytes(const void* plan);
/* arena bytes of one forward + backward pass over `maps` */
int64_t gcl_plan_arena_bytes(void* plan, const gcl_maps_desc* maps_host);
/* Forward pass (training mode: batch statistics, running statistics updated).  x: features of tensor 0
 * [n_rows[level_in of op 0], cin]; params_host[n_params]: DEVICE pointers of the parameters; bn_stats_host[2 * n_bn]:
 * DEVICE pointers running_mean, running_var per BatchNorm.  *y_out_host receives the device pointer (inside the arena)
 * of the last record's output.  The arena must stay untouched until gcl_plan_backward has run. */
int gcl_plan_forward(void* plan, const gcl_maps_desc* maps_host, const float* x, void* const* params_host,
                     void* const* bn_stats_host, void* state, void* arena, int64_t arena_bytes, float** y_out_host,
                     void* stream);
/* Inference pass of the same records (model.eval(), torch.no_grad(): util/misc.py:58-130, scripts/test_kitti.py:141-152):
 * every GCL_OP_CONVBN is ONE gcl_conv_fwd_fused launch -- BatchNorm with running statistics folded into the epilogue as
 * y = relu?(conv * scale + shift (+ residual)) -- the Cin <= 4 first layer is gcl_stem_fwd + gcl_bn_apply(mean, rstd).
 * bn_eval_host[4 * n_bn]: DEVICE pointers scale, shift, mean, rstd per BatchNorm (scale = gamma rsqrt(var + eps),
 * shift = beta - mean scale, rstd = rsqrt(var + eps)).  The packed kernels and their max-abs slots persist in `state`
 * (gcl_plan_eval_state_bytes) from pass to pass: repack != 0 re-measures and re-packs them (first pass, or after the
 * parameters changed).  No backward pass follows; the arena may be released once the output has been consumed. */
int64_t gcl_plan_eval_state_bytes(const void* plan);
int64_t gcl_plan_eval_arena_bytes(void* plan, const gcl_maps_desc* maps_host);
int gcl_plan_forward_eval(void* plan, const gcl_maps_desc* maps_host, const float* x, void* const* params_host,
                          void* const* bn_eval_host, int32_t repack, void* state, void* arena, int64_t arena_bytes,
                          float** y_out_host, void* stream);
/* Backward pass of the forward pass that ran in `arena` (several forward passes of one plan may be outstanding, each in
 * its own arena): the records first_op <= i < last_op in reverse order (the caller may cut the pass into segments,
 * highest records first, e.g. to start a gradient bucket's all-reduce in between).  dy: gradient of the forward output
 * (read by the segment that contains the last record).  grads_host[n_params]: DEVICE pointers that RECEIVE (are
 * overwritten with) the parameter gradients. */
int gcl_plan_backward(void* plan, void* arena, const float* dy, void* const* grads_host, int32_t first_op,
                      int32_t last_op, void* stream);
/* Forget the forward pass parked under `arena` (its output was dropped without a backward pass). */
int gcl_plan_release(void* plan, void* arena);
/* Optional second stream: the weight gradients (needed only by the optimizer) are enqueued there, ordered behind their
 * operands by events, while `stream` continues with the input-gradient chain; every gcl_plan_backward call ends with
 * `stream` waiting for them.  NULL (default) = everything on one stream.  Results do not depend on it. */
int gcl_plan_set_aux_stream(void* plan, void* stream);
/* Plane-only tensors.  A GCL_OP_CONVBN record whose output is at least presplit_min_c channels wide writes its output (forward)
 * and its BatchNorm input gradient (backward) as an fp16 hi/lo plane image in the apply pass.  Where gcl_plan_create's reader
 * analysis shows that every reader takes the image -- convolutions with kernel size > 1 and both widths >= presplit_min_c, in
 * front of the touched-row suffix -- a training pass writes no fp32 twin of that tensor and reserves no arena for it; results
 * are bitwise the same.  A residual operand, an ME.cat input, the plan's output, anything a narrow or kernel_size-1 record
 * reads keeps fp32.  A launch that would read an fp32 form that does not exist returns GCL_ERR_ARG naming the record.
 * gcl_plan_plane_only: flags_host[n_ops], bit 0 = record i's output, bit 1 = its BatchNorm input gradient is plane-only;
 * returns how many tensors are (all words 0 while keep-fp32 is set), negative on a bad argument.
 * gcl_plan_set_keep_fp32(keep != 0): every fp32 twin is written and sized again (for tests and comparisons); it takes
 * effect with the next gcl_plan_arena_bytes / gcl_plan_forward call, and a backward pass follows its own forward pass. */
int gcl_plan_set_keep_fp32(void* plan, int32_t keep);
int gcl_plan_plane_only(const void* plan, int32_t* flags_host, int32_t n_ops);
/* Touched rows.  The plan's touched-row suffix is the longest chain of row-local records -- GCL_OP_ROWNORM, GCL_OP_RELU,
 * kernel_size-1 GCL_OP_CONV -- that ends at the last record and whose input nothing else reads (ResUNetBN2C: conv1_tr, ReLU,
 * final, the row normalisation, behind the ME.cat); gcl_plan_touched_suffix returns its first record, or the number of records
 * when there is none.  A zero row of dy gives a zero row of every gradient inside the suffix and adds nothing to its weight
 * gradients, so a caller that knows which rows of dy can be non-zero (a loss that scatters into selected rows) names them:
 * rows[cap] on the device = the distinct rows, ascending, padded with -1 (gcl_touched_rows makes it).  The NEXT
 * gcl_plan_backward call then gathers those rows, runs the suffix on cap rows through the same entries, and scatters the
 * result into the zero-filled gradient of the suffix's input: that gradient, and everything upstream, is bitwise the dense
 * pass's; the suffix's weight and bias gradients are sums over fewer rows and differ from it in rounding.  The call clears the
 * list (rows must stay allocated until it has returned).  It is ignored -- the dense records run -- without a suffix, when
 * 2 cap >= n_rows, when the call's record range cuts the suffix, or when the pass's arena has no room for it.  A row of dy
 * outside the list that is NOT zero is silently dropped: the list must cover them all.  NULL, 0 withdraws a list.
 *
 * A list handed over BEFORE gcl_plan_forward (training mode; gcl_plan_forward_eval ignores it) makes the forward pass run
 * the suffix on those rows too, under the same rules (a suffix, 2 cap < n_rows, room in the arena -- gcl_plan_arena_bytes
 * keeps sizing for the dense pass, the upper bound): the suffix's input is gathered once into [cap, cin] (its max-abs slot is
 * the dense tensor's, a valid bound), the records run through the same entries with cap rows, and the result is scattered
 * into the zero-filled output.  *y_out is still a dense [n_rows, cout] tensor: THE ROWS OF THE LIST HOLD THE FEATURES, EVERY
 * OTHER ROW IS EXACTLY ZERO -- for a caller that reads nothing else (the group losses above).  The pass parks the list and
 * the compact saved operands with its arena; their padding rows are inert (zero input and activations, y = 0 and norm = 1 out
 * of the row normalisation).  gcl_plan_backward on that arena then gathers dy only and needs no second
 * gcl_plan_set_touched_rows call (one that names the same rows and cap is accepted; another list is GCL_ERR_ARG), so rows must
 * stay allocated until that call has returned.  The features of the listed rows and every gradient differ from the dense
 * pass's in rounding only (the second convolution's input max-abs is taken over fewer rows).  A gcl_plan_backward call whose
 * record range cuts the suffix of such a pass returns GCL_ERR_ARG: there are no dense operands to fall back to -- hand the list
 * over after the forward pass when the backward pass is segmented there.  When the rules are not met the forward pass runs
 * dense and leaves the list for the backward pass, as above. */
int gcl_plan_touched_suffix(const void* plan);
int gcl_plan_set_touched_rows(void* plan, const int32_t* rows, int64_t cap);
/* rows the suffix of the latest gcl_plan_backward call that held the last record ran on: cap, or 0 = the dense records;
 * gcl_plan_suffix_fwd_rows_used: the same for the latest gcl_plan_forward call */
int64_t gcl_plan_suffix_rows_used(const void* plan);
int64_t gcl_plan_suffix_fwd_rows_used(const void* plan);
/* The list for the group losses above: the members index[goff[g] .. goff[g + 1]) of the n_sel selected groups g = sel[s],
 * and the rows of two more index arrays (the negative subsets), as rows[cap] = the distinct rows in [0, n_rows), ascending,
 * then -1; *n_touched (device) = their number -- more than cap means the caller's bound was wrong and the list is cut.
 * Ids outside their array are skipped.  No host synchronisation.  scratch: int32[gcl_touched_rows_scratch_len(n_rows)]. */
int64_t gcl_touched_rows_scratch_len(int64_t n_rows);
int gcl_touched_rows(const int64_t* index, int64_t n_index, const int64_t* goff, int64_t n_groups, const int64_t* sel,
                     int32_t n_sel, const int64_t* rows_a, int32_t n_a, const int64_t* rows_b, int32_t n_b, int64_t n_rows,
                     int32_t* scratch, int32_t* rows, int64_t cap, int32_t* n_touched, void* stream);
/* The two row moves of that path.  gcl_gather_rows: out[j, :] = src[rows[j], :] for j < cap, `pad` in every column where
 * rows[j] is -1 or outside [0, n_src); src is [n_src, c] with row pitch ld floats (a column slice has ld > c), out is
 * contiguous [cap, c].  gcl_scatter_rows: dst[rows[j], :] = src[j, :] for the rows[j] inside [0, n_dst), the others are
 * skipped; dst has row pitch ld, c and ld multiples of 4; a row named twice receives one of its sources. */
int gcl_gather_rows(const float* src, int32_t ld, int64_t n_src, const int32_t* rows, int64_t cap, int32_t c, float pad,
                    float* out, void* stream);
int gcl_scatter_rows(const float* src, const int32_t* rows, int64_t cap, int32_t c, int64_t n_dst, float* dst, int32_t ld,
                     void* stream);
/* With a list, the backward pass does not zero-fill and scatter the gradient of the suffix's input (earlier versions did):
 * it stays compact, [cap, c], through the ME.cat in front of the suffix (split by columns) and into the first BatchNorm
 * backward, which mixes the rows (gcl_bn_bwd_reduce_rows / gcl_bn_bwd_apply_rows: sums and dx bitwise the dense pass's).  A
 * compact gradient that waits at a tensor -- that BatchNorm's residual branch, the cat's other input -- is not handed to the
 * next input-gradient launch as an epilogue operand: the launch runs plain and one launch on cap rows adds it to the output,
 * the same single fp32 addition per element.  Everything upstream stays bitwise the dense pass's.  Any other reader of a
 * compact gradient, and the end of a segmented call, gets it as the dense tensor it stands for (zero fill + scatter).  gcl_scatter_add_rows: dst[rows[j], :] += src[j, :] (src: [cap, c], row pitch src_ld;
 * dst: row pitch ld; the rows of the list are distinct, so one thread owns an element: no atomics).  gcl_row_slots:
 * slots[n] = the position j of row rows[j], -1 for a row that is not on the list. */
int gcl_scatter_add_rows(const float* src, int32_t src_ld, const int32_t* rows, int64_t cap, int32_t c, int64_t n_dst,
                         float* dst, int32_t ld, void* stream);
int gcl_row_slots(const int32_t* rows, int64_t cap, int64_t n, int32_t* slots, void* stream);
/* a stream whose kernels run on the lowest `percent` % of the device's CUs (hipExtStreamCreateWithCUMask) -- measurement hook
 * for the weight-gradient stream (GCL_AUX_CU_PCT); gcl_stream_destroy frees it */
int gcl_stream_create_cu_share(int32_t percent, int32_t low_priority, void** stream_out);
int gcl_stream_destroy(void* stream);
/* Per-launch timing of the convolution launches of the NEXT forward + backward pass (events on `stream`):
 * gcl_plan_profile(plan, 1) arms it; after the stream has been synchronised gcl_plan_profile_read copies up to
 * max_records records of 8 doubles {kind (0 fwd/dx, 1 dW), ms, pairs, cin, cout, n_in, n_out, K | flags} and returns
 * their number. */
int gcl_plan_profile(void* plan, int32_t enable);
int gcl_plan_profile_read(void* plan, double* records_host, int32_t max_records);

/* Elementwise helpers of the plan path (also used by the per-operator path so that both stay bitwise equal):
 * gcl_col_sum: out[c] = sum over rows of x [n, c] (fp64 partials, ordered) -- the bias gradient of `final`
 * (model/resunet.py:165-171); scratch: double[gcl_bn_scratch_len(n, c)]. */
int gcl_col_sum(const float* x, int64_t n, int32_t c, double* scratch, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pair-trainer losses (lib/trainer.py: ContrastiveLossTrainer :198-276, TripletLossTrainer :545-592,
 * HardestTripletLossTrainer :671-744).  F0 [n0, c] and F1 [n1, c] are the features of the two clouds, c <= 64; a
 * "pair" is int64 (row of F0, row of F1).  Nothing here waits for the host; a row id outside its cloud drops its
 * triplet / pair instead of being dereferenced.
 *
 * Positional keys (util/misc.py:43-55): key(r0, r1) = r0 + r1 * seed in wrapping int64.
 * gcl_pair_key_table fills `table` (int64 [cap, 2], cap a power of two >= max(64, 2 n_pos)) with the keys of the
 * n_pos positive pairs (duplicates allowed, n_pos = 0 allowed).  gcl_pair_key_mask probes m candidates:
 *   b == NULL   candidate t is the pair ap[t] itself;
 *   b != NULL   candidate t is the row of column `col` of ap[t] paired with rb = b[b_arg[t]] (b_arg NULL: b[t]) on the
 *               other side, nb = rows in b; b_out (optional) receives rb.
 * keep[t] = 1 iff the candidate's key is not a positive pair's (np.isin negated, lib/trainer.py:211, :583, :716-719).
 * ---------------------------------------------------------------------------------------------- */
int gcl_pair_key_table(const int64_t* pos_pairs, int64_t n_pos, int64_t seed, int64_t* table, int64_t cap, void* stream);
int gcl_pair_key_mask(const int64_t* ap, int32_t col, const int64_t* b, const int32_t* b_arg, int64_t nb, int32_t m,
                      int64_t seed, const int64_t* table, int64_t cap, int64_t* b_out, uint8_t* keep, void* stream);
/* Triplet terms.  Triplet t is the positive pair ap[t] with the negative row neg[t] and tag[t] = side | set << 1:
 *   side 0  anchor F0[ap[t][0]], positive F1[ap[t][1]], negative F1[neg[t]]
 *   side 1  anchor F1[ap[t][1]], positive F0[ap[t][0]], negative F0[neg[t]]
 * term = relu(d(anchor, positive) + margin - d(anchor, negative)), d(x, y) = sqrt(|x - y|^2 + 1e-7) (lib/metrics.py:25).
 * keep (optional uint8 [m]) selects the triplets of the mean.  work: float [gcl_triplet_scratch_len(m)], kept by the
 * caller for the backward pass.  out: float [GCL_TRIPLET_OUT]:
 *   out[0] mean term over the kept triplets (NaN for none), out[1] their number, then for every set s = 0, 1, 2 at
 *   out[2 + 6 s]: kept, all, mean d_pos over kept, mean d_neg over kept, mean d_pos over all, mean d_neg over all.
 * fp64 sums in a fixed order in one workgroup: the forward value is bitwise reproducible.
 * Backward: g = device pointer to the gradient of out[0]; df0 / df1 are caller-zeroed and receive float atomics. */
#define GCL_TRIPLET_OUT 20
int64_t gcl_triplet_scratch_len(int32_t m);
int gcl_triplet_fwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* ap,
                    const int64_t* neg, const uint8_t* tag, const uint8_t* keep, int32_t m, float margin, float* work,
                    float* out, void* stream);
int gcl_triplet_bwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* ap,
                    const int64_t* neg, const uint8_t* tag, const uint8_t* keep, int32_t m, const float* work,
                    const float* out, const float* g, float* df0, float* df1, void* stream);
/* Pair terms over pairs [m, 2] with d2 = |F0[a] - F1[b]|^2; out = {mean term over the kept pairs (NaN for none), their
 * number}; work: float [gcl_pair_terms_scratch_len(m)].  Same backward convention; GCL_PAIR_DIST has no backward pass. */
#define GCL_PAIR_SQ 0        /* d2                                   lib/trainer.py:266 */
#define GCL_PAIR_SQ_POS 1    /* relu(d2 - thresh)                    :459 */
#define GCL_PAIR_NEG 2       /* relu(thresh - sqrt(d2 + eps))^2      :269-270 (eps 1e-4) and :460-461 (eps 1e-7) */
#define GCL_PAIR_DIST 3      /* sqrt(d2 + eps)                       :573 (a statistic) */
int64_t gcl_pair_terms_scratch_len(int32_t m);
int gcl_pair_terms_fwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* pairs,
                       const uint8_t* keep, int32_t m, int32_t mode, float thresh, float eps, float* work, float* out,
                       void* stream);
int gcl_pair_terms_bwd(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* pairs,
                       const uint8_t* keep, int32_t m, int32_t mode, float thresh, float eps, const float* work,
                       const float* out, const float* g, float* df0, float* df1, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Loss backward without float atomics: contribution records and the ordered row sum (csrc/ordered.hip).
 *
 * Every loss backward entry above has an *_emit twin with the same arguments, which writes its contributions as
 * RECORDS instead of adding them into dF: record i = (rec_row[i] int32, rec_val[i][0 .. c) float).  The twin runs the
 * SAME kernel body (the sink is a template parameter), so the values are those the atomic entry hands to atomicAdd.
 *
 * The contribution list of an entry: its (destination row, value[c]) pairs in the order its kernel would issue them if
 * the grid ran one wave at a time in ascending blockIdx, inside a wave in program order.  A record has a FIXED position:
 *   gcl_group_loss_bwd_emit     wave s = selected group s, window rec_off[s] .. rec_off[s + 1): its n_s members in index
 *                               order, then (GCL_LOSS_PAIR) the two drawn members ra, rb
 *   gcl_circle_group_bwd_emit   its n_s members, then the finest member's collected gradient, then (GCL_LOSS_PAIR) ra, rb
 *   gcl_neg_loss_bwd_emit       2 r: sel1[r], 2 r + 1: sel2[arg[r]]
 *   gcl_triplet_bwd_emit        3 t: anchor, 3 t + 1: positive, 3 t + 2: negative
 *   gcl_pair_terms_bwd_emit     t
 * rec_off (int32 [n_sel + 1], an OUTPUT) = the exclusive sums of the window lengths n_s + extra, made on the device;
 * rec_off[n_sel] = the records the entry needs.  The caller sizes the lists from host-known sizes:
 *   gcl_group_loss_records(n_members, n_sel, flags)    = n_members + n_sel * (GCL_LOSS_PAIR ? 2 : 0)
 *   gcl_circle_group_records(n_members, n_sel, flags)  = n_members + n_sel * (GCL_LOSS_PAIR ? 3 : 1)
 *   gcl_neg_loss_records(m) = 2 m,  gcl_triplet_records(m) = 3 m,  gcl_pair_terms_records(m) = m        (0 for counts <= 0)
 * with n_members = the sum of the selected groups' sizes (or any bound of it, such as the length of `index` when the
 * selected groups are distinct).  n_rec = the capacity of the lists the caller passes: the three per-item entries refuse
 * an n_rec below their count; the two group entries cannot know n_members without a host read and DROP a record whose
 * slot is at or past n_rec (nothing is written out of bounds; rec_off[n_sel] > n_rec tells).
 *
 * Rules of a list:
 *   - every entry first sets rec_row[0 .. n_rec) = -1.  A contribution the atomic kernel skips -- a wave that returns
 *     early (both upstream gradients zero or both hinges inactive, an inactive hinge of the negative term or of a
 *     triplet / pair), a keep == 0 item, a row id outside its cloud, the GCL_LOSS_PAIR slots of a group whose positive
 *     term has no gradient -- and every unused slot therefore is a record with row -1; its value is not written.
 *   - a value vector is recorded WHOLE.  The atomic kernels skip a lane whose value is exactly 0.f (the members' and the
 *     finest member's contributions), the record keeps the zero: the ordered result may differ from an atomic one in the
 *     sign of a zero and in nothing else.
 *   - the pair family writes TWO lists, one per cloud (rec_row0 / rec_val0 -> dF0, rec_row1 / rec_val1 -> dF1), both with
 *     the slots above and n_rec records each: a contribution stands in the list of the cloud it goes to, the same slot
 *     of the other list is -1.  (A single list with a cloud tag would make the reduction filter; two lists reduce with
 *     two plain calls.)
 *   - several entries into one dF (group loss, then the negative term): one list, the entries' windows one after the other
 *     in call order (pass each entry its part of rec_row / rec_val).
 *
 * gcl_ordered_row_sum: for every row r in [0, n_rows) named by at least one record,
 *     dF[r] = fl(... fl(fl(dF[r] + v_1) + v_2) ... + v_k)   in fp32, over the row's records in ascending list position;
 * the sum starts from what dF[r] holds (the atomic entries' "accumulates into a pre-filled buffer"); rows no record
 * names are not written; records with a row < 0 or >= n_rows are skipped.  By construction this is one of the results
 * the atomic kernels may produce -- and the same bits on every run.  c <= 64, n_rows < 2^31.  No host read; integer
 * atomics only count and place, and a row's record ids are put in ascending order (a bitmap per window of
 * gcl_ordered_row_sum_window() consecutive ids, in LDS, by the wave that owns the row) before anything is added; a row
 * may be named by any number of records.  scratch: int32 [gcl_ordered_row_sum_scratch_len(n_rec, n_rows)] =
 * 2 + 2 n_rows + 3 n_rec (0 when either count is <= 0).
 * ---------------------------------------------------------------------------------------------- */
int64_t gcl_group_loss_records(int64_t n_members, int32_t n_sel, int32_t flags);
int gcl_group_loss_bwd_emit(const float* f, int32_t c, const int64_t* index, const int64_t* goff,
                            const uint8_t* finest_flag, const int64_t* sel, int32_t n_sel, float pos_thresh,
                            float finest_thresh, int32_t flags, const int32_t* pairpos, const float* gpos,
                            const float* gfin, int32_t* rec_off, int32_t* rec_row, float* rec_val, int32_t n_rec,
                            void* stream);
int64_t gcl_circle_group_records(int64_t n_members, int32_t n_sel, int32_t flags);
int gcl_circle_group_bwd_emit(const float* f, int32_t c, const int64_t* index, const int64_t* goff,
                              const uint8_t* finest_flag, const int64_t* sel, int32_t n_sel, float pos_thresh,
                              float finest_thresh, float log_scale, int32_t flags, const int32_t* pairpos,
                              const float* gpos, const float* gfin, const float* gmean, int32_t* rec_off,
                              int32_t* rec_row, float* rec_val, int32_t n_rec, void* stream);
int64_t gcl_neg_loss_records(int32_t m);
int gcl_neg_loss_bwd_emit(const float* f, int32_t c, const int64_t* sel1, const int64_t* sel2, const int32_t* arg,
                          const float* dmin, const uint8_t* keep, int32_t m, float thresh, const float* out,
                          const float* gneg, int32_t* rec_row, float* rec_val, int32_t n_rec, void* stream);
int64_t gcl_triplet_records(int32_t m);
int gcl_triplet_bwd_emit(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* ap,
                         const int64_t* neg, const uint8_t* tag, const uint8_t* keep, int32_t m, const float* work,
                         const float* out, const float* g, int32_t* rec_row0, float* rec_val0, int32_t* rec_row1,
                         float* rec_val1, int32_t n_rec, void* stream);
int64_t gcl_pair_terms_records(int32_t m);
int gcl_pair_terms_bwd_emit(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, const int64_t* pairs,
                            const uint8_t* keep, int32_t m, int32_t mode, float thresh, float eps, const float* work,
                            const float* out, const float* g, int32_t* rec_row0, float* rec_val0, int32_t* rec_row1,
                            float* rec_val1, int32_t n_rec, void* stream);
int32_t gcl_ordered_row_sum_window(void);
int64_t gcl_ordered_row_sum_scratch_len(int32_t n_rec, int64_t n_rows);
int gcl_ordered_row_sum(const int32_t* rec_row, const float* rec_val, int32_t n_rec, int32_t c, int64_t n_rows,
                        int32_t* scratch, float* df, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FPFH descriptors (csrc/fpfh.hip): what open3d's estimate_normals + compute_fpfh_feature give, made on the device for
 * the `descriptor: fpfh` arm of the SC2-PCR benchmark (scripts/SC2_PCR/dataset.py:66-74 only loads them).  xyz [n, 3]
 * is a concatenation of n_clouds clouds; offsets (DEVICE int64 [n_clouds + 1], ascending, offsets[0] = 0,
 * offsets[n_clouds] = n) gives their rows, and a point's neighbours come from its own cloud only.  All arithmetic is fp64.
 *
 * gcl_fpfh_cell_keys: keys[i] = (cloud, cx, cy, cz) of point i on a grid whose edge is just above `radius`.  The caller
 * sorts them ascending (ties in any order) and passes the sorted keys and the permutation (`order[s]` = row of the
 * s-th key) to gcl_fpfh_neighbours with the SAME radius.
 * gcl_fpfh_neighbours: idx[i] = the rows of the <= max_nn nearest points with d2 <= r2 (the point itself included) in
 * ascending (d2, row) order, -1 behind them; cnt[i] their number.  d2 = (dx dx + dy dy) + dz dz with every operation
 * rounded on its own, r2 = double(radius)^2.  Exact for any number of in-radius candidates.
 * gcl_fpfh_normals: the unit eigenvector of the smallest eigenvalue of the covariance of the cnt[i] listed points,
 * turned towards viewpoint (float [n_clouds, 3], NULL: the origin); (0, 0, 1) for fewer than 3 points.
 * gcl_fpfh_spfh: spfh [n, 33] from the list entries 1 .. cnt - 1 (open3d's ComputePairFeatures, 11 bins per feature,
 * integer counts times 100 / (cnt - 1)).
 * gcl_fpfh_combine: fpfh [n, 33] = per feature 100 / sum times the sum over the entries 1 .. cnt - 1 with d2 != 0 of
 * spfh[entry] / d2, plus spfh[i]; normalize != 0: each row divided by (its 2-norm + 1e-6).  fpfh must not alias spfh.
 * An idx entry outside [0, n) is skipped, never dereferenced; cnt is clamped to [0, max_nn].  None of the calls needs
 * scratch memory or waits for the host.
 * ---------------------------------------------------------------------------------------------- */
#define GCL_FPFH_MAX_NN 128
#define GCL_FPFH_MAX_CLOUDS 32767
#define GCL_FPFH_BINS 33
int gcl_fpfh_cell_keys(const float* xyz, int64_t n, const int64_t* offsets, int32_t n_clouds, float radius, int64_t* keys,
                       void* stream);
int gcl_fpfh_neighbours(const float* xyz, int64_t n, const int64_t* offsets, int32_t n_clouds, const int64_t* sorted_keys,
                        const int64_t* order, float radius, int32_t max_nn, int32_t* idx, int32_t* cnt, void* stream);
int gcl_fpfh_normals(const float* xyz, int64_t n, const int32_t* idx, const int32_t* cnt, int32_t max_nn,
                     const float* viewpoint, const int64_t* offsets, int32_t n_clouds, float* normals, void* stream);
int gcl_fpfh_spfh(const float* xyz, const float* normals, int64_t n, const int32_t* idx, const int32_t* cnt, int32_t max_nn,
                  float* spfh, void* stream);
int gcl_fpfh_combine(const float* xyz, const float* spfh, int64_t n, const int32_t* idx, const int32_t* cnt, int32_t max_nn,
                     int32_t normalize, float* fpfh, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Validation step for a ragged batch of B pairs (csrc/valpose.hip; lib/colocation_trainer.py:306-379 runs it once per
 * pair on the host).  src / tgt (float [total, 3]) are the matched points of all pairs, pair b owning the rows
 * offsets[b] .. offsets[b + 1] - 1 (DEVICE int64 [B + 1], ascending, within [0, total]); a pair whose offsets fall outside
 * that range is treated as empty.  One launch each, no atomics, nothing read back: a pair's numbers are bitwise the same on
 * every run and whatever else the batch holds.
 *
 * gcl_irls_pose_batch: the algorithm of util/transform_estimation.py:97-126 (est_quad_linear_robust) in fp64: n_iter (20)
 * re-weighted Gauss-Newton steps on w^2 [-[p]x | I] x = w^2 (q - p) through the 6 x 6 normal equations (partial
 * pivoting), the step applied as Rz Ry Rx + t, w = par / (|p - q| + par) with par = par0 (1.0) halved at every multiple
 * of halve_every (5) steps, trans = step trans.  weight (float [total], NULL: ones) are the weights of the first step.
 * T (double [B, 16], row-major 4 x 4) maps src onto tgt; status (int32 [B]) is 0, or 1 when a pair is empty or a step's
 * system had a zero or non-finite pivot (below 2^-40 of the largest entry of its column counts as zero) or a non-finite
 * solution: T is the identity then.
 * Scratch: gcl_irls_pose_scratch_len(total) = 3 * total doubles (the current points); NULL only when total = 0.
 *
 * gcl_val_stats_batch: out (double [B, 6]) = loss, rte, rre, hit_ratio, n_corr, status per pair.
 *   loss       mean over the pair's rows of xyz0 (float [total0, 3], rows offsets0[b] .. offsets0[b + 1] - 1) of
 *              min(|T_est x - T_gt x|, max_dist)                                        (lib/metrics.py:13-19, corr_dist)
 *   rte        |t_est - t_gt|;   rre  arccos((trace(R_est^T R_gt) - 1) / 2), NOT clamped: NaN passes through
 *   hit_ratio  mean over the pair's correspondences of sqrt(|T_gt a - b|^2 + 1e-6) < thresh      (:397-400); the count
 *              is exact and the quotient rounded to float32, which is the reference's float32 mean bit for bit
 *   status     a copy of status[b] (NULL: 0).  Means over zero rows are 0.
 * T_est / T_gt are double [B, 16]; all arithmetic is fp64, sums in a fixed order.  No scratch.
 * ---------------------------------------------------------------------------------------------- */
int64_t gcl_irls_pose_scratch_len(int64_t total);
int gcl_irls_pose_batch(const float* src, const float* tgt, int64_t total, const int64_t* offsets, int32_t B,
                        const float* weight, int32_t n_iter, double par0, int32_t halve_every, double* scratch, double* T,
                        int32_t* status, void* stream);
int gcl_val_stats_batch(const float* src, const float* tgt, int64_t total, const int64_t* offsets, const float* xyz0,
                        int64_t total0, const int64_t* offsets0, int32_t B, const double* T_est, const double* T_gt,
                        const int32_t* status, double max_dist, double thresh, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point-to-point ICP for a ragged batch of n_pairs scan pairs (csrc/icp.hip): open3d's registration_icp with
 * TransformationEstimationPointToPoint, restated from its published source (DESIGN.md "ICP" holds the semantics and the two
 * deviations), as the pair loaders refine the odometry pose with it (lib/data_loaders.py:447-474,
 * lib/complement_data_loader.py:369-399) and scripts/SC2_PCR/benchmark_utils.py:40-56 offers it.  All arithmetic is fp64.
 *   xyz0 [total0, 3], xyz1 [total1, 3]   sources and targets; pair b owns the rows offsets[b] .. offsets[b + 1] - 1
 *   offsets0_host / offsets1_host        HOST int64 [n_pairs + 1], ascending from 0 to total0 / total1 (<= 2^31 - 1), checked
 *                                        before anything is launched; offsets0 / offsets1: the same numbers on the DEVICE
 *   sorted_keys, order                   gcl_fpfh_cell_keys(xyz1, total1, offsets1, n_pairs, (float)max_correspondence_distance)
 *                                        sorted ascending, and the permutation (`order[s]` = target row of the s-th key)
 *   init  double [n_pairs, 16]           row-major 4 x 4, T_0
 * Iteration k pairs every source point p = T_k x with the target row of its own pair that minimises
 * d2 = (dx dx + dy dy) + dz dz (every operation rounded) among those with d2 <= double(max_correspondence_distance)^2, ties
 * to the lowest row; n_corr, fitness = n_corr / n_source and inlier_rmse = sqrt(sum d2 / n_corr) are the result under T_k;
 * the update is the Kabsch solution U without scale over the pairs (p, q) and T_k+1 = U T_k.  The result under T_0 is
 * evaluated first; then up to max_iteration times: update, evaluate, stop when |d fitness| < relative_fitness and
 * |d inlier_rmse| < relative_rmse.  Outputs per pair:
 *   T      double [n_pairs, 16]   the final transformation (init's fourth row is kept)
 *   stats  double [n_pairs, 4]    fitness, inlier_rmse, n_corr under T; the number of updates applied
 *   status int32 [n_pairs]        0; 1: an empty source or target or no correspondence at some evaluation; 2: one or two
 *                                 correspondences (the solution is not unique).  1 and 2 stop the pair with the T and the
 *                                 result of that evaluation; they are looked at before the convergence test.
 *   corr   int32 [total0]         optional: the target row WITHIN the pair's own target under the final T, or -1
 * The call enqueues one set-up launch and max_iteration + 1 pairs of launches (step, update); the blocks of a finished pair
 * return at once.  Nothing is read back, the host never waits, there are no atomics: a pair's T, stats and corr are bitwise
 * the same alone, anywhere in any batch and on every run.  scratch: gcl_icp_scratch_bytes(total0, total1, n_pairs) bytes (16 per target
 * for the targets in cell order, 136 per 256 source rows for the partial sums); the query returns 0 for arguments out of
 * range.  1 <= n_pairs <= GCL_FPFH_MAX_CLOUDS, 0 <= max_iteration <= 1 000 000.
 * ---------------------------------------------------------------------------------------------- */
int64_t gcl_icp_scratch_bytes(int64_t total0, int64_t total1, int32_t n_pairs);
int gcl_icp_register_batch(const float* xyz0, const int64_t* offsets0_host, const int64_t* offsets0, const float* xyz1,
                           const int64_t* offsets1_host, const int64_t* offsets1, int32_t n_pairs,
                           const int64_t* sorted_keys, const int64_t* order, double max_correspondence_distance,
                           const double* init, int32_t max_iteration, double relative_fitness, double relative_rmse,
                           void* scratch, double* T, double* stats, int32_t* status, int32_t* corr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multiway registration (csrc/multiway.hip, csrc/posegraph.h): what lib/complement_data_loader.py:407-516 does with open3d
 * after the pairwise ICPs, restated from open3d's published source (DESIGN.md "Multiway registration" holds the semantics).
 * All arithmetic is fp64; nothing is read back, there are no atomics: a pair's matrix and a graph's result are bitwise the
 * same alone, anywhere in a batch and on every run.
 *
 * gcl_info_matrix_batch: get_information_matrix_from_point_clouds for n_pairs pairs in the layout of
 * gcl_icp_register_batch (xyz0 / xyz1, host and device offsets, the sorted keys and order of a gcl_fpfh_cell_keys grid built
 * at THIS call's (float)max_correspondence_distance).  transformation: DEVICE double [n_pairs, 16].  The correspondence of
 * source row i is the ICP's: the nearest target row of the same pair to p = T x_i with d2 <= distance^2, ties to the lowest
 * row.  info (double [n_pairs, 36], row-major 6 x 6, rotation part first) = sum over the correspondences of G^T G, G's rows
 * being (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1) of the TARGET point (x, y, z); info[5][5] is the number
 * of correspondences.  An empty cloud or a pair without correspondences gives the zero matrix (all bits zero: the negated
 * entries are formed as 0 - v).  Three launches.
 * scratch: gcl_info_scratch_bytes(total0, total1, n_pairs) bytes (0 for arguments out of range).
 *
 * gcl_multiway_compose: the pose graphs of the reference's full_registration.  Graph g owns the nodes node_offsets[g] ..
 * node_offsets[g + 1] - 1 (n of them, 1 .. 8) and the edges edge_offsets[g] .. (n (n - 1) / 2 of them: every pair s < t in
 * the order s = 0 .. n - 1, t = s + 1 .. n - 1); offsets are DEVICE int32 [n_graphs + 1].  T_icp (double [total_edges, 16])
 * are the pairs' transformations in that order.  Writes nodes (double [total_nodes, 16]: node 0 = I, node k =
 * inverse(T_icp(k - 1, k) ... T_icp(0, 1)), the rigid inverse), edges (int32 [total_edges, 2]: s, t) and uncertain (int32
 * [total_edges]: t != s + 1).  One thread per graph.
 *
 * gcl_posegraph_optimize_batch: global_optimization with GlobalOptimizationLevenbergMarquardt, one workgroup per graph (at
 * most 8 nodes and 28 edges; the 48 x 48 system lives in LDS).  nodes / edges / edge_T / edge_info / uncertain as above
 * (device; edge_info double [total_edges, 36]).  params: HOST double [12] = max_correspondence_distance,
 * edge_prune_threshold, preference_loop_closure, reference_node, then the convergence criteria max_iteration (<= 1000),
 * min_relative_increment, min_relative_residual_increment, min_right_term, min_residual, max_iteration_lm (<= 100),
 * upper_scale_factor, lower_scale_factor.  Outputs: poses (double [total_nodes, 16]), confidence (double [total_edges]),
 * kept (int32 [total_edges]), stats (double [n_graphs, 3]: linear solves of pass 1, of pass 2, the final residual) and
 * status (int32 [n_graphs]): 0; 1: the line-process weight is 0 (no edge carries a correspondence); 2: a non-finite input;
 * 3: a pivot of the L D L^T was not positive; for 1 .. 3 the input poses are returned, every edge kept at confidence 1.
 * 4: the graph's structure is out of range (the caller validates it; nothing else is written for that graph).
 * ---------------------------------------------------------------------------------------------- */
int64_t gcl_info_scratch_bytes(int64_t total0, int64_t total1, int32_t n_pairs);
int gcl_info_matrix_batch(const float* xyz0, const int64_t* offsets0_host, const int64_t* offsets0, const float* xyz1,
                          const int64_t* offsets1_host, const int64_t* offsets1, int32_t n_pairs, const int64_t* sorted_keys,
                          const int64_t* order, const double* transformation, double max_correspondence_distance,
                          void* scratch, double* info, void* stream);
int gcl_multiway_compose(const int32_t* node_offsets, const int32_t* edge_offsets, int32_t n_graphs, int32_t total_nodes,
                         int32_t total_edges, const double* T_icp, double* nodes, int32_t* edges, int32_t* uncertain,
                         void* stream);
int gcl_posegraph_optimize_batch(const double* nodes, const int32_t* node_offsets, const int32_t* edges,
                                 const int32_t* edge_offsets, const double* edge_T, const double* edge_info,
                                 const int32_t* uncertain, int32_t n_graphs, int32_t total_nodes, int32_t total_edges,
                                 const double* params, double* poses, double* confidence, int32_t* kept, double* stats,
                                 int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The complement pair loaders' neighbourhood cloud (PairComplementKittiDataset / PairComplementNuscenesDataset.__getitem__,
 * lib/complement_data_loader.py:576-628, :1028-1060): for every SIDE of a batch (a pair's centre scan; n_sides <= 64, side
 * 2 b + s of sample b) its complement scans are moved into the centre frame, cropped to the centre scan's range and
 * concatenated in order.  All arithmetic is float32 with every product and sum rounded on its own, apply_transform's
 * q = ((x0 r0 + x1 r1) + x2 r2) + t with the transform rounded to float32 first, the squared range (x^2 + y^2) + z^2.
 *   aug_dev / aff_dev      the tables of gcl_cloud_affines, DEVICE double[>= n_sides][12]: only aug's `rotated` column and the
 *                          T_s = [R | R (-centroid)] of a rotated side are read; the scale is NOT applied here (the reference
 *                          crops before it scales, :623-628 before :656-662).
 * gcl_nghb_range_max       max_dev float[n_clouds]: over cloud c of gcl_voxel_coords_multi's layout (cloud_offsets_host: HOST
 *                          int64[n_clouds + 1]) the maximum of the squared range of f32(T_c) x, or of x where the cloud is not
 *                          rotated; 0 for an empty cloud.  An LDS tree per 1024 points, then an integer atomic max on the bit
 *                          pattern: the same bits alone, anywhere in a batch, on every run.  One memset, one launch.
 * gcl_nghb_flags           one thread per complement point.  cmpl [pc, 3]: the raw complement scans of all sides, side after
 *                          side; scan_offsets_host: HOST int64[n_scans + 1] point offsets; scan_side_host: HOST int32[n_scans],
 *                          the side of every scan, not descending; n_scans <= GCL_NGHB_MAX_SCANS; scan_aff_dev: DEVICE
 *                          double[n_scans][12], row-major 3 x 4, complement -> centre (list_M).  moved [pc, 3] = f32(M_k) x,
 *                          moved again by f32(T_s) where side s is rotated (the second transform acts on the rounded result of
 *                          the first); flags int32[pc] = 1 where the squared range of `moved` is strictly below max_dev[s].
 *                          pc = 0 launches nothing.
 * gcl_nghb_compact         out [kept, 3] = the flagged rows of `moved` in order (capacity pc rows); side_offsets_host: HOST
 *                          int64[n_sides + 1] point offsets of the sides in cmpl; kept_dev: DEVICE int32[n_sides + 1] = kept
 *                          points of every side, then their total.  scratch: int32[gcl_nghb_scratch_len(pc)] = pc +
 *                          pc / 2048 + 64 (0 for pc <= 0).  One scan (gcl_exclusive_scan_i32) and one launch; pc = 0 zeroes
 *                          kept_dev.
 * Every entry returns GCL_ERR_ARG before anything is launched for a negative count, more than 64 clouds / sides, offsets that
 * do not ascend from 0 to the point count, or a null pointer where the sizes need one.
 * ---------------------------------------------------------------------------------------------- */
#define GCL_NGHB_MAX_SCANS 256
int gcl_nghb_range_max(const float* xyz, int64_t p, const int64_t* cloud_offsets_host, int32_t n_clouds, const double* aug_dev,
                       const double* aff_dev, float* max_dev, void* stream);
int gcl_nghb_flags(const float* cmpl, int64_t pc, const int64_t* scan_offsets_host, const int32_t* scan_side_host,
                   int32_t n_scans, int32_t n_sides, const double* scan_aff_dev, const double* aug_dev, const double* aff_dev,
                   const float* max_dev, float* moved, int32_t* flags, void* stream);
int64_t gcl_nghb_scratch_len(int64_t pc);
int gcl_nghb_compact(const float* moved, const int32_t* flags, int64_t pc, const int64_t* side_offsets_host, int32_t n_sides,
                     int32_t* scratch, float* out, int32_t* kept_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCL_AMD_H */
