/*
 * sgs_hip.h -- C ABI of libsgs_hip.so, the MI355X (gfx950) implementation of the SGS-GNN
 * hot path: edge scoring -> exponential-race top-q edge sampling -> weighted sparse GCN
 * forward/backward (+ gate and losses).
 *
 * The reference (anonymousauthors001/SGS-GNN) has no native/FFI layer: its boundary is the
 * Python call sites of training_hybrid.py / sampling.py / model.py.  Each entry point below
 * names the reference lines whose device work it replaces; INTEGRATION.md shows the ctypes
 * binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host"; tensors are dense row-major;
 *   - `edge_index` is PyG's int64 [2,E] layout: src = edge_index, dst = edge_index + E;
 *   - inputs are borrowed, outputs are caller-allocated; no entry point allocates, frees,
 *     synchronises the device or keeps global state -> all are HIP-graph capturable;
 *   - scratch memory comes from the caller: query `*_workspace_bytes`, pass `ws, ws_bytes`;
 *   - work is enqueued on `stream` (a hipStream_t cast to void*; NULL = default stream);
 *   - return value: SGS_OK or a negative SGS_E* code; `sgs_last_error()` gives the
 *     thread-local message (the reference only ever raises RuntimeError/ValueError: the
 *     Python host layer turns a non-zero code into RuntimeError).
 */
#ifndef SGS_HIP_H_
#define SGS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGS_ABI_VERSION 1

#define SGS_OK 0
#define SGS_EINVAL (-1)    /* bad argument (shape, null pointer, q > E ...) */
#define SGS_EWORKSPACE (-2) /* workspace too small */
#define SGS_EHIP (-3)      /* a HIP runtime call failed */

typedef void* sgs_stream_t;

int sgs_abi_version(void);
const char* sgs_last_error(void);

/* ------------------------------------------------------------------------------------
 * Counter-based randomness (replaces torch's global generator draws).
 *   sgs_exp_noise   : noise[e] ~ Exp(1), Philox4x32-10 keyed by `seed`, counter (e, stream_id).
 *                     The sampler generates exactly these values in-register when it is given
 *                     noise == NULL (reference: the exponential_() inside torch.multinomial,
 *                     sampling.py:96, training_hybrid.py:47).
 *   sgs_dropout_keep: keep[r*cols+c] in {0,1}, P(keep)=1-p, hash of (seed, site, r, c); the
 *                     same bits the fused kernels apply (reference: nn.Dropout at
 *                     model.py:107,121,160).  Only tests need the materialised form.
 * ---------------------------------------------------------------------------------- */
/* HIP-graph replay support: seeds are passed by value and therefore frozen in a captured graph.  When a
 * device word is registered here, every RNG-consuming kernel uses seed + 0x9E3779B97F4A7C15 * (*epoch_dev);
 * a captured increment of that word makes every replay draw fresh noise and dropout masks.  NULL (the
 * default) = seeds used exactly as given.  Process-wide; the word must outlive all launches that read it. */
int sgs_rng_set_epoch_buffer(const uint64_t* epoch_dev);
int sgs_exp_noise(uint64_t seed, uint64_t stream_id, int64_t E, float* noise, sgs_stream_t stream);
int sgs_dropout_keep(uint64_t seed, uint32_t site, int64_t rows, int64_t cols, float p, uint8_t* keep,
                     sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * One captured step for partitions of ANY size (HIP-graph replay of training_hybrid.py:29-187's loop body without one capture
 * per partition).  Sizes and pointers are launch arguments, frozen at capture; two entry points lift that:
 *   sgs_dyn_edges_set : while a device word is registered, the entry points whose grids run over the CANDIDATE edges of a partition
 *                       (sgs_sample_topq, sgs_edge_score_fwd, the dense part of sgs_st_weights_bwd, sgs_gather_by_eid /
 *                       sgs_scatter_by_eid) use n = min(their size argument, *word) rows and treat the argument as the CAPACITY
 *                       (grid size, row stride of `edge_index`, buffer and workspace sizes).  A drawn subgraph has q < E edges,
 *                       so calls over it are unaffected.  Process-wide, read at launch (= capture) time; NULL = off.
 *                       Everything downstream of the draw is sized by q and N, which a run fixes.
 *   sgs_stage_segments: the batch hand-over of training_hybrid.py:42 (`batch.to(device)`) for resident partitions: ONE launch copies
 *                       up to sgs_stage_max_segments() spans from a partition's resident arrays into the static buffers a
 *                       captured step reads, pads each destination tail with a 32-bit word (zero rows for padded nodes, E for
 *                       the row pointers past N, ...) and writes up to 4 dims words (the E that sgs_dyn_edges_set points at).
 *                       desc_host [n_segments][5] int64, HOST memory, read during the call: {src, dst, src_bytes, dst_bytes >=
 *                       src_bytes, pad word}; spans are whole 4-byte words.  HBM-bound: 16 B per lane, 16 KiB per workgroup.
 * ---------------------------------------------------------------------------------- */
int sgs_dyn_edges_set(const int64_t* n_edges_dev);
int sgs_stage_max_segments(void);
int sgs_stage_segments(const int64_t* desc_host, int64_t n_segments, int64_t* dims_dev, const int64_t* dims_host, int64_t n_dims,
                       sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Multi-partition batches: the collate of ClusterLoader(cluster_data, batch_size=k) (main.py:63-65 uses batch_size=1) for a graph
 * that is resident on the device -- the union of k partitions with the cut edges between them restored.
 *
 * The whole graph is held as a row-sorted CSR whose nodes are grouped by partition: full_ptr [N+1] int64, full_col [E] int64,
 * full_prob [E] (may be NULL).  Partition p owns the node range [node_ptr[p], node_ptr[p+1]).  A group is k ranges in ASCENDING
 * order: ranges_host [k][2] int64 = {lo, hi}, HOST memory, read during the call and passed to the kernels by value (as
 * sgs_stage_segments does with its descriptors): no allocation, no synchronisation and no device-side table that would have to be
 * refilled per batch, so the call can be captured.  k <= sgs_cluster_collate_max_parts() (32).
 *
 * Batch node r is the r-th node of the concatenated ranges (n_b of them).  Every edge (s, d) of the whole graph with both endpoints
 * in the ranges is emitted with local ids, ordered by (local src, local dst): relabelling is monotone because the group is ascending,
 * so a row's kept columns keep their order.  Outputs: edge_index_out [2, E_b] int64; prob_out [E_b] = full_prob gathered (bit for
 * bit; may be NULL); eid_out [E_b] int64 = position of each emitted edge in full_col (may be NULL).  Per-node BYTE attributes (the
 * boolean masks: their per-partition slices are not whole aligned words, so they cannot go through sgs_stage_segments like x and y):
 * attr_in [n_attr][N] -> attr_out [n_attr][n_b], n_attr <= 4, may be 0.
 *
 * E_b is the HOST's edge count of the batch (the caller knows it without a read-back from a P x P block count table;
 * sgs_cluster_collate_count gives it otherwise: it runs the count and the scan only and writes the total to *total_dev).  If
 * mismatch_dev (device int32, may be NULL) is given and the device count differs from E_b, the word is set to 1 (it is never
 * cleared here); nothing is written outside [0, E_b) of any output either way.
 *
 * Launches: count per row (one wave per row; also the byte attributes), scan, fill -- the row squeeze and the single-workgroup scan
 * that sgs_nbr_induced_count / _fill run too (csrc/batch_rows.h).  Rows longer than 1024 columns are walked by the 16 waves of their
 * workgroup together.  Integer work and gathers only; no atomics.  ws: sgs_cluster_collate_workspace_bytes(n_b) bytes, 8-byte
 * aligned: the int64 rowptr [n_b + 1], which holds the row counts until the scan turns them into offsets in place.
 * Errors (SGS_EINVAL, message in sgs_last_error): k < 1 or k > cap, ranges unsorted / overlapping / not n_b nodes
 * in total, n_b or E_b >= 2^31, workspace too small.
 * ---------------------------------------------------------------------------------- */
int sgs_cluster_collate_max_parts(void);
size_t sgs_cluster_collate_workspace_bytes(int64_t n_b);
int sgs_cluster_collate_count(const int64_t* full_ptr, const int64_t* full_col, const int64_t* ranges_host, int64_t k, int64_t n_b,
                              int64_t* total_dev, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_cluster_collate(const int64_t* full_ptr, const int64_t* full_col, const float* full_prob, const int64_t* ranges_host, int64_t k,
                        int64_t n_b, int64_t E_b, int64_t* edge_index_out, float* prob_out, int64_t* eid_out, const uint8_t* attr_in,
                        uint8_t* attr_out, int64_t n_attr, int64_t N, int32_t* mismatch_dev, void* ws, size_t ws_bytes,
                        sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K0 / K2 / K3: fused exponential-race top-q edge sampler + stable compaction.
 *
 * Replaces, in one call:
 *   mode SGS_SAMPLE_LEARNED  sampling.py:91-96,134-139 (`gumbel_softmax_sampling`: normalise,
 *                            mix with the degree prior unless istest, multinomial w/o
 *                            replacement, one-hot mask) + training_hybrid.py:83,86
 *                            (`edge_index[:, mask]`, `edge_probs_full[mask]`);
 *   mode SGS_SAMPLE_PRIOR    training_hybrid.py:46-48 (softmax(batch.prob), multinomial,
 *                            column gather) -- output is in ORIGINAL edge order (the
 *                            reference's race order is irrelevant to every consumer).
 *
 *   s_e   = p_e / (sum(p) + 1e-12)                      (learned)
 *         = (1-c) * s_e + c * prior_e                   (learned, prior != NULL, i.e. !istest)
 *         = exp(p_e - max p) / sum exp(p - max p)       (prior mode: softmax of `p`)
 *   key_e = s_e / noise_e        IEEE fp32 divide, noise ~ Exp(1)
 *   selected = the q largest keys; ties broken towards the LOWEST edge id.
 *
 * `noise` may be NULL: then noise_e is generated in-register exactly as sgs_exp_noise(seed,
 * stream_id) would.  Outputs (any may be NULL except mask): mask[E] (0/1 bytes, torch.bool
 * compatible), sampled_eid[q] ascending edge ids, sampled_edge_index[2,q], sampled_p[q] =
 * p[sampled_eid], stats[4] = {Z (sum p or sum exp), max (prior mode), threshold key, #ties
 * taken at the threshold}.  keys_out[E] (optional) receives the fp32 keys (tests only).
 * p == NULL (mode LEARNED, prior == NULL): uniform weights, i.e. a uniformly random q-subset of the edges -- the selection
 * behind `random_edge_sampling` (sampling.py:159-163, torch.randperm(E)[:q]), emitted in original edge order.
 *
 * Order of the keys: by the uint32 BIT PATTERN of the fp32 key, not by its float value.  Every key the sampler computes is >= +0 and
 * finite, where the two orders agree.  For other bits (reachable through negative or NaN inputs) the bit order holds: a key with bit
 * 31 set (-0 included) ranks above every positive key, a NaN ranks by its bits, -0 and +0 are different keys.
 * Z and max are reduced in one fixed order (per 2048-edge chunk, then over the chunk partials): stats[0] and stats[1] are the same bits
 * on the fused small-E path, the general path (E > 2 097 152, q == 0, q == E) and the phase API below, for any shard count.
 * q == 0 / q == E: nothing / everything is selected without a race: no keys are computed (keys_out is left untouched), stats[2] =
 * stats[3] = 0, and q == 0 leaves sampled_eid / sampled_edge_index / sampled_p untouched.
 * Under sgs_dyn_edges_set (capacity = the E argument, live = the registered word; 0 < q < E <= 2 097 152 is required, else SGS_EINVAL):
 * every output is what the plain call with E = live returns on the first `live` entries, edge_index keeping the capacity as its row
 * stride; mask[live .. capacity) and keys_out[live .. capacity) are NOT written (the caller owns their contents).  q <= live is the
 * caller's responsibility.  (tests/test_gpu_sampler_kernels.py pins all of this.)
 *
 * sgs_gather_columns: out[:, j] = edge_index[:, idx[j]] (sampling.py:163 with an explicit index vector, e.g. the first q
 * entries of a given permutation); indices outside [0, E) give (-1, -1).
 * ---------------------------------------------------------------------------------- */
#define SGS_SAMPLE_LEARNED 0
#define SGS_SAMPLE_PRIOR 1

size_t sgs_sample_topq_workspace_bytes(int64_t E);
int sgs_sample_topq(int mode, const float* p, const float* prior, double degree_bias_coef,
                    const float* noise, uint64_t seed, uint64_t stream_id, int64_t E, int64_t q,
                    const int64_t* edge_index, uint8_t* mask, int64_t* sampled_eid,
                    int64_t* sampled_edge_index, float* sampled_p, float* stats, float* keys_out,
                    void* ws, size_t ws_bytes, sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * sgs_sample_topq_cover: the same draw under the NODE-COVERING rule (opt-in; sgs_sample_topq itself is unchanged).  The rule alters WHICH
 * edges are drawn, not how a drawn edge is weighted or differentiated (sgs_st_weights_fwd / _bwd take the selected ids as they are).
 *
 *   key_e    = the fp32 key of sgs_sample_topq, bit for bit (every mode, explicit or in-register noise);
 *   forced   : for every node i, the candidate edge with dst == i and src != i that has the largest key, ties to the lowest edge id
 *              (a node without such an edge has none; self-loops never count).  M = number of forced edges;
 *   boosted  = float_as_uint(key_e), bit 31 set when e is forced (keys >= 0, so the bit is free);
 *   selected = the q largest boosted keys, ties to the lowest edge id; compaction in original edge order.
 *
 * Hence exactly q edges are selected; M <= q: every node with a non-loop in-edge keeps its best one and the other q - M edges are the
 * q - M largest keys of the rest; M > q: the q largest-keyed forced edges; M == 0: the plain draw.  q == 0 / q == E select nothing /
 * everything as sgs_sample_topq does (no keys are computed then; cover_info is still written).  E == 0 returns at once and writes
 * nothing.
 *
 * in_ptr [N + 1] / in_src / in_eid [E]: the destination-row CSR of the candidate graph as sgs_graph_build emits it.  Outputs as
 * sgs_sample_topq, with: stats[2] = the threshold key with the flag bit cleared, stats[3] = the number of ties taken at the BOOSTED
 * threshold, keys_out = the unboosted keys (bitwise the plain call's), cover_info[2] (int32, may be NULL) = {M, number of forced
 * edges selected = min(M, q)}.
 *
 * Launches: the plain draw's, plus one kernel after the key pass (per row: gather the keys of the row's entries, 64-bit max of
 * (key bits << 32 | ~edge id), set bit 31 of the winner, move its count in the top-digit histogram from bin b to bin b + 1024 --
 * integer atomics, aggregated per workgroup first) and one finishing workgroup (M, the reported threshold).  All counting is integer:
 * the draw is run-to-run and launch-geometry invariant.  sgs_sample_topq_cover_variant(N, E) -> lanes that share one row in that
 * kernel: 4 (E < 8 N), 16 (E < 64 N) or 64; a row of more than 32 entries per lane (128 / 512 / 2048) is taken by the whole
 * 256-thread workgroup instead.  A pure host function.
 *
 * Capturable as sgs_sample_topq is (no allocation, synchronisation or read-back) and honours sgs_dyn_edges_set with the same capacity
 * semantics: the caller guarantees that in_ptr describes the LIVE edges, rows past the live nodes being empty (pointers padded with
 * the live E, as sgs_stage_segments pads them).  E < 2^31 and N < 2^31 (int32 CSR).
 * ---------------------------------------------------------------------------------- */
size_t sgs_sample_topq_cover_workspace_bytes(int64_t E, int64_t N);
int sgs_sample_topq_cover_variant(int64_t N, int64_t E);
int sgs_sample_topq_cover(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise,
                          uint64_t seed, uint64_t stream_id, int64_t E, int64_t q, const int64_t* edge_index,
                          int64_t N, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                          uint8_t* mask, int64_t* sampled_eid, int64_t* sampled_edge_index, float* sampled_p,
                          float* stats, float* keys_out, int32_t* cover_info, void* ws, size_t ws_bytes, sgs_stream_t stream);

int sgs_gather_columns(const int64_t* edge_index, int64_t E, const int64_t* idx, int64_t q, int64_t* out, sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Phase API of the sampler for EDGE-SHARDED draws (config 5: one graph, edges split over R ranks in
 * contiguous shards whose boundaries are multiples of sgs_sampler_chunk()).  Between phases the host
 * runs the collectives (torch.distributed over RCCL): all-gather of the per-chunk partial sums
 * (reduced by sgs_sampler_shard_finalize in the single-GPU order => bit-identical normaliser),
 * all-reduce(sum) of each 2048-bin digit histogram, all-gather of the per-rank (#greater, #equal)
 * counts.  Noise is keyed by the GLOBAL edge id (edge_offset + local id), ties go to the lowest global
 * ids, so the selected set is identical for every rank count (tests: 1 vs 2 vs 3 ranks).
 *   keys buffer: first region of the caller's workspace (sgs_sampler_shard_workspace_bytes), uint32 [E].
 *   state: 16 bytes of device memory, zeroed by the caller before pass 0.
 * ---------------------------------------------------------------------------------- */
size_t sgs_sampler_shard_workspace_bytes(int64_t E_local);
int64_t sgs_sampler_chunk(void);
int sgs_sampler_shard_partials(int stage, const float* p, int64_t E, const float* scal, float* part, sgs_stream_t stream);
int sgs_sampler_shard_finalize(int stage, const float* part_all, int64_t nblk_all, float* scal, sgs_stream_t stream);
int sgs_sampler_shard_keys(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise,
                           uint64_t seed, uint64_t stream_id, int64_t edge_offset, int64_t E, const float* scal,
                           uint32_t* keys, float* keys_out, uint32_t* hist, sgs_stream_t stream);
int sgs_sampler_shard_hist(const uint32_t* keys, int64_t E, int pass, const void* state, uint32_t* hist,
                           sgs_stream_t stream);
int sgs_sampler_select(uint32_t* hist, int pass, int64_t q, void* state, sgs_stream_t stream);
int sgs_sampler_shard_count(const uint32_t* keys, int64_t E, const void* state, uint32_t* counts, void* ws,
                            size_t ws_bytes, sgs_stream_t stream);
int sgs_sampler_shard_compact(const uint32_t* keys, int64_t E, const void* state, int64_t ties_local, int64_t q_local,
                              int64_t edge_offset, const float* p, const int64_t* edge_index_local, uint8_t* mask,
                              int64_t* sampled_eid, int64_t* sampled_edge_index, float* sampled_p, void* ws,
                              size_t ws_bytes, sgs_stream_t stream);

/* Straight-through weights of sampling.py:137-138,155 for the selected edges:
 *   w_j = clamp(p_e * ((1 - s_e) + s_e), 0, 1),  e = sampled_eid[j]   (forward value)
 * and its exact autograd backward wrt p (s depends on every p through sum(p)):
 *   dp_e += [e selected] g_e ((1 - s_e) + s_e) + ... (see DESIGN.md "straight-through").
 * Used by --pipeline straight_through and by evaluate.py.  prior == NULL <=> istest.
 * Under sgs_dyn_edges_set the backward writes exactly +0 to grad_p[live .. E); the selected ids must lie below the live count. */
int sgs_st_weights_fwd(const float* p, const float* prior, double degree_bias_coef, const float* stats,
                       const int64_t* sampled_eid, int64_t E, int64_t q, float* w, sgs_stream_t stream);
size_t sgs_st_weights_bwd_workspace_bytes(int64_t E, int64_t q);
int sgs_st_weights_bwd(const float* p, const float* prior, double degree_bias_coef, const float* stats,
                       const int64_t* sampled_eid, const float* grad_w, int64_t E, int64_t q, float* grad_p,
                       void* ws, size_t ws_bytes, sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K4: graph preparation for the GCN layers = the bookkeeping half of PyG's
 * add_remaining_self_loops + gcn_norm, done ONCE per sampled graph and shared by both layers,
 * forward and backward (the reference redoes it inside every GCNConv call: model.py:107-111,
 * 159-161).
 *
 * For the n_edges edges (src,dst) of `edge_index` [2,n_edges] over N nodes, builds both CSR
 * orientations, rows ordered by edge id (deterministic, so every floating-point row sum is
 * run-to-run reproducible):
 *   in_ptr[N+1],  in_src[n_edges],  in_eid[n_edges]    rows = dst   (forward aggregation)
 *   out_ptr[N+1], out_dst[n_edges], out_eid[n_edges]   rows = src   (transposed / backward)
 *   loop_eid[N] = id of the LAST existing self-loop edge of node i, or -1  (PyG: an existing
 *                 loop keeps its weight, otherwise the added loop has weight 1)
 * Self-loop edges stay in the CSRs (the edge scorer's backward needs them); the norm kernel
 * gives them weight 0 there and routes them through the loop term.  int32 indices.
 * ---------------------------------------------------------------------------------- */
size_t sgs_graph_build_workspace_bytes(int64_t n_edges, int64_t N);
int sgs_graph_build(const int64_t* edge_index, int64_t n_edges, int64_t N, int32_t* in_ptr, int32_t* in_src,
                    int32_t* in_eid, int32_t* out_ptr, int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid,
                    void* ws, size_t ws_bytes, sgs_stream_t stream);

/* CSR of a sampled subgraph from its PARENT's CSR (sgs_graph_build of the partition, built once and cached): the draw keeps
 * a subset of the parent's edges in their original order, so the child rows are the parent rows with the unselected entries
 * squeezed out and edge ids renumbered by rank in `sampled_eid` (ascending parent edge ids, as sgs_sample_topq emits them):
 * no atomics, no per-row sort, three launches.  mask [E_parent] u8; child arrays sized as for sgs_graph_build(q, N).
 * Result is identical to sgs_graph_build on the compacted edge list. */
size_t sgs_graph_filter_workspace_bytes(int64_t E_parent, int64_t N);
int sgs_graph_filter(const int32_t* pin_ptr, const int32_t* pin_src, const int32_t* pin_eid, const int32_t* pout_ptr,
                     const int32_t* pout_dst, const int32_t* pout_eid, int64_t E_parent, int64_t N, const uint8_t* mask,
                     const int64_t* sampled_eid, int64_t q, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid, int32_t* out_ptr,
                     int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid, void* ws, size_t ws_bytes, sgs_stream_t stream);

/* sgs_graph_build for an edge list that is SORTED BY SOURCE (what a draw over a row-sorted edge list emits; the reference's loaders all
 * produce row-sorted lists, and sampling.py keeps the order: edge_index[:, mask]).  The out-CSR is then the list itself; the in-CSR is ONE
 * stable radix sort of (dst, (src, edge id)) -- at whole-graph scale (config 5: q = 22.9 M drawn edges of 114.6 M) this replaces
 * sgs_graph_filter's passes over the PARENT's CSR.  Same arrays as sgs_graph_build.  `unsorted` (device word, may be NULL): set to 1 if
 * the list turns out not to be sorted by source (the arrays are then meaningless), 0 otherwise. */
size_t sgs_graph_build_src_sorted_workspace_bytes(int64_t n_edges, int64_t N);
int sgs_graph_build_src_sorted(const int64_t* edge_index, int64_t n_edges, int64_t N, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid,
                               int32_t* out_ptr, int32_t* out_dst, int32_t* out_eid, int32_t* loop_eid, int32_t* unsorted, void* ws,
                               size_t ws_bytes, sgs_stream_t stream);

/* gcn_norm forward (PyG gcn_norm, add_self_loops=True, flow source_to_target):
 *   loopw_i = w[loop_eid_i] or 1;  deg_i = loopw_i + sum_{e=(j->i), j!=i} w_e;  dis = deg^-1/2 (inf -> 0)
 *   what_in[k]  = dis[src] * w * dis[dst] in dst-CSR order,  what_out[k] the same in src-CSR order
 *   what_loop[i] = dis_i * loopw_i * dis_i
 * w == NULL means unit weights. */
int sgs_gcn_norm_fwd(const float* w, int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* in_src,
                     const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                     const int32_t* loop_eid, float* dis, float* loopw, float* what_in, float* what_out,
                     float* what_loop, sgs_stream_t stream);

/* Edge-sharded gcn_norm (config 5): each rank sums the weights of its own in-edges
 * (sgs_gcn_degree_partial), the host all-reduces the [N] vector, and sgs_gcn_norm_from_degree continues
 * with deg_i = 1 + degsum_i (the added self loop counts once; graphs with existing (i,i) edges are not
 * supported in sharded mode).  sgs_bias_act applies the layer epilogue AFTER the all-reduce of the
 * partial aggregates:  Y = act(X + bias), act as in sgs_spmm_csr. */
int sgs_gcn_degree_partial(const float* w, int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* in_src,
                           const int32_t* in_eid, float* degpart, sgs_stream_t stream);
int sgs_gcn_norm_from_degree(const float* w, const float* degsum, int64_t n_edges, int64_t N, const int32_t* in_ptr,
                             const int32_t* in_src, const int32_t* in_eid, const int32_t* out_ptr,
                             const int32_t* out_dst, const int32_t* out_eid, float* dis, float* loopw, float* what_in,
                             float* what_out, float* what_loop, sgs_stream_t stream);
int sgs_bias_act(const float* X, const float* bias, int64_t N, int64_t D, int act, float p_drop, uint64_t seed,
                 uint32_t site, float* Y, sgs_stream_t stream);
/* The same on a BLOCK of rows of a larger matrix (node-block sharding): X, Y [n_rows, D] hold rows row_offset .. row_offset + n_rows - 1,
 * and the dropout rows are those global ids, so the mask equals the unsharded one's. */
int sgs_bias_act_rows(const float* X, const float* bias, int64_t n_rows, int64_t D, int64_t row_offset, int act, float p_drop,
                      uint64_t seed, uint32_t site, float* Y, sgs_stream_t stream);

/* GraphSAGE mean aggregation for the GSAGE scorer (model.py:47-89, PyG SAGEConv aggr='mean'): per-entry
 * weights 1 / indeg(dst) in both CSR orders, to be used with sgs_spmm_csr (diag = NULL).
 * sgs_degree_prior_logits: the argument of the softmax in datasets.py:141-156 (`add_degree`),
 * E^-1/2 / (colcount[row_e] + rowcount[col_e] + 1e-10); the softmax itself is the sampler's prior mode,
 * or torch.softmax when the materialised `data.prob` is wanted. */
int sgs_mean_weights(int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_dst,
                     float* what_in, float* what_out, sgs_stream_t stream);
int sgs_degree_prior_logits(const int64_t* edge_index, int64_t E, int64_t N, const int32_t* in_ptr,
                            const int32_t* out_ptr, float* logits, sgs_stream_t stream);

/* gcn_norm backward: from gw_hat[e] = dL/d(what_e) (edge-id order) and gloop[i] = dL/d(what_loop_i)
 * to dL/dw_e, through both the message weight and the degree normalisation:
 *   dw_e = gw_hat_e dis_s dis_t + Hn_t,            Hn_t = -1/2 dis_t^3 G_t
 *   G_t  = sum_{e' into t} gw_hat_e' w_e' dis_src + sum_{e' out of t} gw_hat_e' w_e' dis_dst
 *          + 2 gloop_t loopw_t dis_t
 * (every existing self-loop edge (i,i) gets gloop_i dis_i^2 + Hn_i -- also a duplicate whose weight was
 * overwritten, which is what autograd does for PyG's `loop_attr[idx] = edge_attr[inv_mask]`). */
size_t sgs_gcn_norm_bwd_workspace_bytes(int64_t N);
int sgs_gcn_norm_bwd(const float* w, const float* gw_hat, const float* gloop, int64_t n_edges, int64_t N,
                     const float* dis, const float* loopw, const int32_t* in_ptr, const int32_t* in_src,
                     const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                     const int32_t* loop_eid, const int64_t* edge_index, float* dw, void* ws, size_t ws_bytes,
                     sgs_stream_t stream);
/* ... with up to two upstream gradients summed on read (gw_hat2 / gloop2: the second GCN layer over the same normalisation; both or neither)
 * and another consumer's d w added on the way out (dw_add, optional; may be dw itself) -- the add kernels autograd would launch. */
int sgs_gcn_norm_bwd_sum(const float* w, const float* gw_hat, const float* gloop, const float* gw_hat2, const float* gloop2, const float* dw_add,
                         int64_t n_edges, int64_t N, const float* dis, const float* loopw, const int32_t* in_ptr, const int32_t* in_src,
                         const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                         const int32_t* loop_eid, const int64_t* edge_index, float* dw, void* ws, size_t ws_bytes, sgs_stream_t stream);

/* Split form of sgs_gcn_norm_bwd for edge-sharded graphs: Hn (per node) is linear in the edge contributions, so
 * each rank computes its partial Hn (gloop non-zero only on the rank that owns the self-loop term), the host
 * all-reduces Hn [N], and the per-edge pass finishes locally. */
int sgs_gcn_norm_bwd_node(const float* w, const float* gw_hat, const float* gloop, int64_t n_edges, int64_t N,
                          const float* dis, const float* loopw, const int32_t* in_ptr, const int32_t* in_src,
                          const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                          float* Hn, sgs_stream_t stream);
int sgs_gcn_norm_bwd_edge(const float* gw_hat, const float* gloop, int64_t n_edges, int64_t N, const float* dis,
                          const int32_t* loop_eid, const int64_t* edge_index, const float* Hn, float* dw,
                          sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K5: weighted CSR SpMM with fused epilogue (GCNConv propagate + bias, F.relu, nn.Dropout;
 * model.py:107-111,159-161):
 *   Y[i,:] = act( sum_{k in row i} val[k] X[col[k],:] + diag[i] X[i,:] + bias )
 * act: identity | ReLU | ReLU then counter-based dropout(p, seed, site) (see sgs_dropout_keep).
 * Forward uses (in_ptr, in_src, what_in, what_loop); the transposed product of backward,
 * dX = A_hat^T dZ, is the same call with (out_ptr, out_dst, what_out, what_loop).
 * diag / bias may be NULL; nnz = ptr[N] (known to the caller; picks the row-per-workgroup kernel for
 * few long rows).  X is the already linearly transformed feature matrix [N,D]
 * (the dense X W^T is a library GEMM on the host side).
 * ---------------------------------------------------------------------------------- */
#define SGS_ACT_NONE 0
#define SGS_ACT_RELU 1
#define SGS_ACT_RELU_DROPOUT 2
int sgs_spmm_csr(const float* X, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col, const float* val,
                 const float* diag, const float* bias, int act, float p_drop, uint64_t seed, uint32_t site, float* Y,
                 sgs_stream_t stream);

/* SDDMM over the same CSR (gradient wrt the normalised weights):
 *   g[eid[k]] = <A[i,:], B[col[k],:]> for k in row i;  gdiag[i] = <A[i,:], B[i,:]>  (gdiag may be NULL) */
int sgs_sddmm_csr(const float* A, const float* B, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col,
                  const int32_t* eid, float* g, float* gdiag, sgs_stream_t stream);

/* Which kernel the two calls above launch for a shape (pure host functions; the launchers switch on their result; aligned16 != 0: both
 * dense operands are 16-byte aligned).  Code = kind * 1000 + VEC * 100 + W:  kind 0 = W lanes per row (LPR), kind 1 = a workgroup of
 * W waves per row (NW);  VEC = floats per lane and load (4 needs D % 4 == 0 and the alignment).  DESIGN.md section 5 has the table. */
int sgs_spmm_csr_variant(int64_t N, int64_t D, int64_t nnz, int aligned16);
int sgs_sddmm_csr_variant(int64_t N, int64_t D, int64_t nnz, int aligned16);

/* Long rows in the row-block SpMM kernels (kind 1 above, and every call below that gathers as they do: sgs_spmm_csr_next,
 * sgs_spmm_csr_bwd_prev, the two-job forms, sgs_spmm_csr_multi).  On (the default), a graph of at most 4096 rows launches kernels in
 * which a row of sgs_spmm_long_rows_threshold() entries or more loads its (col, val) stream 64 entries per wave at a time and keeps
 * two batches of X rows in flight; every sum keeps its order, so the outputs are bitwise the same either way.  Off launches the plain
 * kernels (for A/B timing and tests).  sgs_spmm_long_rows_set returns the previous value; the value is read when a call launches, so a
 * captured graph keeps the kernels it was captured with.  sgs_spmm_long_rows_active(N, D): 1 iff a call on N rows of width D would launch
 * the long-row kernels now (the switch is on and the shape is inside their range).  All three are host-only and need no GPU. */
int sgs_spmm_long_rows_set(int on);
int sgs_spmm_long_rows_threshold(void);
int sgs_spmm_long_rows_active(int64_t N, int64_t D);

/* dZ = dY * act'(Y) for the fused epilogue above (Y is the layer OUTPUT: Y > 0 iff kept and
 * positive, so no mask is stored);  colsum: out[d] = sum_i A[i,d]  (bias gradient). */
int sgs_act_bwd(const float* dY, const float* Y, int64_t n, int act, float p_drop, float* dZ, sgs_stream_t stream);
size_t sgs_colsum_workspace_bytes(int64_t N, int64_t D);
int sgs_colsum(const float* A, int64_t N, int64_t D, float* out, void* ws, size_t ws_bytes, sgs_stream_t stream);
/* Both in one pass (one launch for partition-sized N): dZ = dY * act'(Y) written, colsum[d] = sum_i dZ[i,d] -- the activation and bias
 * gradients of one layer's backward (autograd of model.py:159-161).  ws: sgs_colsum_workspace_bytes(N, D). */
int sgs_act_bwd_colsum(const float* dY, const float* Y, int64_t N, int64_t D, int act, float p_drop, float* dZ, float* colsum, void* ws,
                       size_t ws_bytes, sgs_stream_t stream);

/* Which kernels sgs_colsum (fused_act = 0) / sgs_act_bwd_colsum (fused_act != 0) launch (pure host function):
 * kind * 1000000 + F * 100000 + rows * 100 + RG;  kind 1 = colsum_small, 2 = colsum_small_v4, 3 = vecsum_small, 4 = colsum_partial over
 * `rows` rows per chunk + colsum_final<RG>;  F = 1 with the activation backward (in the kernel for kinds 1, 2; a launch of its own else). */
int sgs_colsum_variant(int64_t N, int64_t D, int fused_act);

/* GCN layer pairs at partition scale: one SpMM launch carries the neighbouring layer's row-local work.
 * sgs_gcn_pair_ok(N, nnz, D): 1 iff sgs_spmm_csr takes its row-block path (N <= 65536, nnz >= 16 N) and 0 < D <= 512 (rows of width
 *   D are kept in LDS); the two calls below accept exactly these shapes.
 * sgs_spmm_csr_next: Y = sgs_spmm_csr(X, ...) bitwise, and Z = Y Wn^T in fp32 (Wn [Dn, D] row-major: the next layer's weight; Z [N, Dn]).
 * sgs_spmm_csr_bwd_prev: dX = A_hat^T dZ bitwise as sgs_spmm_csr over the out-CSR (dZ, dX [N, D]);  colsum[d] = sum_i dZ[i, d]
 *   (NULL: skipped; bitwise sgs_colsum for N <= 2048);  and with W != NULL (W [D, Dp] row-major: the weight that made this layer's
 *   input) dZp = (dX W) * act'(Yp) [N, Dp] in fp32, act' as in sgs_act_bwd (Yp [N, Dp]: the previous layer's output). */
int sgs_gcn_pair_ok(int64_t N, int64_t nnz, int64_t D);
int sgs_spmm_csr_next(const float* X, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col, const float* val,
                      const float* diag, const float* bias, int act, float p_drop, uint64_t seed, uint32_t site, const float* Wn, int64_t Dn,
                      float* Y, float* Z, sgs_stream_t stream);
int sgs_spmm_csr_bwd_prev(const float* dZ, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col, const float* val,
                          const float* diag, const float* W, int64_t Dp, const float* Yp, int act, float p_drop, float* dX, float* dZp,
                          float* colsum, sgs_stream_t stream);

/* Two-job forms of the GNN head's two forward launches: job a and job b are two graphs over the same N rows (the learned and the random
 * subgraph of a sampled step) that share everything but their CSR, weights, dropout seed and outputs.  One launch (gridDim.y = 2) runs
 * both; each job's outputs are bitwise what the single-job call writes.
 * sgs_gcn_dual_ok(N, nnz_a, nnz_b, D, Dn): 1 iff both jobs pass sgs_gcn_pair_ok(N, nnz, D), Dn > 0 and both select the same kernel
 *   variant by their size (nnz >= 256 N or not, for both); the layer-2 call over rows of width Dn then takes its row-block path for both
 *   jobs as well.  (The variants also depend on 16-byte alignment of X and Y, which the calls check per job.)
 * sgs_spmm_csr_next_dual: per job sgs_spmm_csr_next(X, ..., Wn, Dn, Y_j, Z_j) with the shared X, bias, act, p_drop, site, Wn.
 * sgs_spmm_csr_dual: per job sgs_spmm_csr(X_j, ..., Y_j) on its row-block path with the shared bias, act, p_drop, site.
 * Both return SGS_EINVAL and launch nothing when either job is not a row-block shape or the two jobs would select different kernel
 * variants: the caller then makes the two single-job calls. */
int sgs_gcn_dual_ok(int64_t N, int64_t nnz_a, int64_t nnz_b, int64_t D, int64_t Dn);
int sgs_spmm_csr_next_dual(const float* X, int64_t N, int64_t D, const float* bias, int act, float p_drop, uint32_t site, const float* Wn,
                           int64_t Dn, int64_t nnz_a, const int32_t* ptr_a, const int32_t* col_a, const float* val_a, const float* diag_a,
                           uint64_t seed_a, float* Y_a, float* Z_a, int64_t nnz_b, const int32_t* ptr_b, const int32_t* col_b,
                           const float* val_b, const float* diag_b, uint64_t seed_b, float* Y_b, float* Z_b, sgs_stream_t stream);
int sgs_spmm_csr_dual(const float* X_a, const float* X_b, int64_t N, int64_t D, const float* bias, int act, float p_drop, uint32_t site,
                      int64_t nnz_a, const int32_t* ptr_a, const int32_t* col_a, const float* val_a, const float* diag_a, uint64_t seed_a,
                      float* Y_a, int64_t nnz_b, const int32_t* ptr_b, const int32_t* col_b, const float* val_b, const float* diag_b,
                      uint64_t seed_b, float* Y_b, sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K1b: fused edge scorer (model.py:29-34 / 115-122 `_edge_score`; never materialises the
 * reference's [E,2H] feature or [E,H] hidden tensors):
 *   p_e = sigmoid( w2 . drop(relu( W1 [x_s*x_d | x_s-x_d] + b1 )) + b2 ),  x = codes rows
 * Algebraic split  W1 [x*y | x-y] = W1a (x*y) + U[s] - U[d]  with U = codes W1b^T a node-level
 * library GEMM done by the caller, so the per-edge contraction is H x H; it runs on the f32
 * matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).
 *   codes, U [N,H] f32; W1 = fc1.weight [H,2H]; b1 [H]; w2 = fc2.weight [H]; b2 [1].
 *   4 <= H <= 256 with H % 4 == 0, or 256 < H <= 1024 with H % 32 == 0 (sgs_edge_score_hidden_supported).  The wide sizes run a
 *   chunked kernel of their own (the hidden units swept 256 at a time, fixed-order fc2 accumulation) in sgs_edge_score_fwd,
 *   sgs_edge_score_fwd_paired, sgs_edge_score_bwd_core and the endpoint-dropout pair; every other scorer entry point (bf16 mode,
 *   mask form, fused backward, dfeat) stays H = 128 or 256 as its _supported predicate says.  Dropout on the hidden layer is
 *   counter-based, row = edge_id_offset + local edge id (edge_id_offset = 0 unless the edge list is a shard of a larger graph).
 * ws: sgs_edge_score_workspace_bytes(N, H, E).
 *
 * sgs_edge_score_bwd_core runs over an explicit list of active edges (hybrid / two-pass: the q
 * sampled edges -- every other edge has exactly zero upstream gradient; NULL = all E edges in
 * order) and RECOMPUTES the hidden layer instead of storing it.  It writes, per active row j:
 *   dv[j,:]  = dL/d(fc1 pre-activation)       dz[j] = grad_p_j p_j (1-p_j)  (sum -> d b2)       feat[j,:] = x_s * x_d
 * and, per tile of sgs_edge_score_bwd_tile() (= 64) consecutive active rows, ONE row of
 *   hdz_part[tile,:] = sum_{j in tile} dz_j * hidden_j          (rows sum to d w2; hidden is never written per edge)
 * from which the host forms  d W1a = dv^T feat (sgs_gemm_tn),  d b1 = colsum(dv),  d w2 = colsum(hdz_part),
 * dfeat = dv W1a (library GEMM) and the two endpoint reductions below.
 *
 * sgs_endpoint_reduce: out[v,:] = sum_{k in out-row v} sign_out M_out[out_eid[k],:] (* T[out_dst[k],:])
 *                               + sum_{k in in-row v}  sign_in  M_in[in_eid[k],:]   (* T[in_src[k],:])
 * over the CSRs of the ACTIVE edge list (sgs_graph_build): the scatter of per-edge gradient rows
 * to both endpoints as a deterministic gather (no float atomics).  T may be NULL.
 *   d codes (direct) = reduce(dfeat, dfeat, T = codes, +1, +1);   d U = reduce(dv, dv, NULL, +1, -1).
 * ---------------------------------------------------------------------------------- */
size_t sgs_edge_score_workspace_bytes(int64_t N, int64_t H, int64_t E);   /* E = 0 for the backward core */
/* 1 if the fp32 scorer entry points above take hidden size H: 4 <= H <= 256 with H % 4 == 0, or 256 < H <= 1024 with H % 32 == 0;
 * else 0.  Host only (callable without a GPU). */
int sgs_edge_score_hidden_supported(int64_t H);
int sgs_edge_score_get_variant(void);          /* the overrides currently set (-1 = automatic) */
int sgs_edge_score_get_bwd_variant(void);
void sgs_edge_score_set_bwd_variant(int variant); /* backward core: -1 = automatic (4 at H % 128 == 0 and >= 65 536 active rows, else 0), 0 = LDS-tiled, 3 = 64-edge streaming loop (A/B: measured slower), 4 = bf16x6 loop; ignored at H > 256 */
int sgs_edge_score_bwd_tile(void);              /* active rows per hdz_part row (64) */
void sgs_edge_score_set_variant(int variant);   /* forward kernel: -1 = automatic (default: when E >= 65 536, 4 if H % 128 == 0 else 3; below that 1),
                                                  * 0 = LDS-tiled, 1 = register-streaming (32-edge wave tile), 2 = weight-stationary
                                                  * persistent, 3 = register-streaming with a 64-edge wave tile, 4 = bf16x6: exact
                                                  * 3-way bf16 splits of both operands, six v_mfma_f32_32x32x16_bf16 per fp32
                                                  * product (fp32-faithful; H % 128 == 0, else 3); all give the same p to fp32
                                                  * rounding.  Both switches are A/B selectors among the H <= 256
                                                  * kernels: at H > 256 they are ignored (one chunked kernel) */
int sgs_edge_score_fwd(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index, int64_t E,
                       int64_t edge_id_offset, const float* W1, const float* b1, const float* w2, const float* b2,
                       float p_drop, uint64_t seed, uint32_t site, float* p_out, void* ws, size_t ws_bytes,
                       sgs_stream_t stream);
/* Paired forward.  fc1's edge-level half W1a (x_s * x_d) is symmetric in the endpoints, so on an undirected graph stored in both
 * directions (every dataset of the reference: datasets.py:189-190) an edge and its reverse share that contraction bit for bit; they
 * differ in the sign of U[s] - U[d] and in their dropout rows.  sgs_edge_mates pairs the edges (mate[e] = id of (dst_e -> src_e)
 * or -1; mutual, one to one; needs the src-CSR of sgs_graph_build), the caller lists the canonical edges (mate < 0 or e < mate)
 * and sgs_edge_score_fwd_paired runs the H x H contraction for those M edges only, finishing both scores of a pair in its
 * epilogue: p_out [E] equals sgs_edge_score_fwd's bit for bit.  H = 128, 256 or any wide size 256 < H <= 1024, H % 32 == 0
 * (ask sgs_edge_score_paired_supported).
 * Under sgs_dyn_edges_set the live M is read from word 1 of the registered dims (word 0 = live E). */
size_t sgs_edge_mates_workspace_bytes(int64_t n_edges);
int sgs_edge_mates(const int64_t* edge_index, int64_t n_edges, int64_t N, const int32_t* out_ptr, const int32_t* out_dst,
                   const int32_t* out_eid, int32_t* mate, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_paired_supported(int64_t H);
int sgs_edge_score_fwd_paired(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index, int64_t E,
                              int64_t edge_id_offset, const int32_t* canon, int64_t M, const int32_t* mate, const float* W1, const float* b1,
                              const float* w2, const float* b2, float p_drop, uint64_t seed, uint32_t site, float* p_out, void* ws,
                              size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_core(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index,
                            int64_t E, int64_t edge_id_offset, const int64_t* active_eid, int64_t n_active, const float* grad_p,
                            const float* W1, const float* b1, const float* w2, const float* b2, float p_drop,
                            uint64_t seed, uint32_t site, float* dv, float* hdz_part, float* dz, float* feat, void* ws,
                            size_t ws_bytes, sgs_stream_t stream);
/* dfeat [n,H] = dv [n,H] . W1[:, :H]: the gradient wrt the Hadamard features x_s * x_d that the scorer backward (model.py:29-34 under
 * autograd) forms from sgs_edge_score_bwd_core's dv.  The forward's bf16x6 loop as a row GEMM (fp32-faithful, see
 * sgs_edge_score_set_variant); H = 128 or 256 only -- ask sgs_edge_score_bwd_dfeat_supported, other sizes use a library GEMM.
 * Workspace: sgs_edge_score_workspace_bytes(0, H, 0). */
int sgs_edge_score_bwd_dfeat_supported(int64_t H);
int sgs_edge_score_bwd_dfeat(const float* dv, int64_t n, int64_t H, const float* W1, float* dfeat, void* ws, size_t ws_bytes,
                             sgs_stream_t stream);

/* The MASK form of the scorer backward (H = 128 or 256; sgs_edge_score_bwd_bits_supported).  With v the fc1 pre-activation,
 *   dv[r, h] = dz[r] * w2[h] * [dropout(relu(v))[r, h] > 0] / (1 - p)            (autograd of model.py:31-33 / 119-121)
 * is a 0 / 1 matrix times a row and a column factor, so the core writes ONE BIT per entry -- dvbits [n, H/32], bit h of row r in word
 * h / 32 -- instead of the fp32 [n, H] matrix, and the three consumers take bits + dz + w2:
 *   sgs_edge_score_bwd_dfeat_bits   dfeat = dv W1a            = dz[r] * (bits[r, :] . diag(w2 / (1 - p)) W1a)
 *   sgs_gemm_tn_mask                d W1a = dv^T feat, d b1   = diag(w2 / (1 - p)) (bits^T (diag(dz) feat))
 *   sgs_endpoint_reduce_pair_bits   d U[v] = w2 / (1 - p) * (sum_out - sum_in) dz[e] bits[e, :]   (+ the d codes half, as sgs_endpoint_reduce_pair)
 * A 0 / 1 operand is exact in bf16: the two contractions issue 3 bf16 MFMA products per fp32 product (the other operand's exact 3-way
 * split) instead of 6, still fp32-faithful.  Other arguments as sgs_edge_score_bwd_core / _bwd_dfeat / sgs_endpoint_reduce_pair. */
int sgs_edge_score_bwd_bits_supported(int64_t H);
/* No recompute at all when the FORWARD kept the mask (sgs_edge_score_fwd_mask: the bf16x6 forward, paired when canon / mate are given, that
 * also writes maskbits [E, H/32] for every scored edge; scores bit-identical to the plain forward):
 *   sgs_edge_score_bwd_prep        per active row r (edge e): dz[r] = grad_p[r] p[e] (1 - p[e]), dvbits[r, :] = maskbits[e, :],
 *                                  feat[r, :] = codes[src e, :] * codes[dst e, :]                       (one HBM-bound pass)
 *   sgs_edge_score_dw2_from_parts  d fc2.weight[h] = 1/(1-p) * ( sum_k W1a[h,k] T[h,k] + sum_v U[v,h] R[v,h] + b1[h] c[h] ) from the
 *                                  consumers' results before their factors: T = C_raw and c = colsum_raw of sgs_gemm_tn_mask,
 *                                  R = out_U_raw of sgs_endpoint_reduce_pair_bits (exact algebra: hidden = mask * (W1a feat + U[s] - U[d] + b1) / (1-p))
 * then sgs_edge_score_bwd_dfeat_bits, sgs_gemm_tn_mask, sgs_endpoint_reduce_pair_bits as after sgs_edge_score_bwd_core_bits. */
int sgs_edge_score_fwd_mask(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index, int64_t E,
                            int64_t edge_id_offset, const int32_t* canon, int64_t M, const int32_t* mate, const float* W1, const float* b1,
                            const float* w2, const float* b2, float p_drop, uint64_t seed, uint32_t site, float* p_out, uint32_t* maskbits,
                            void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_prep(const float* codes, int64_t N, int64_t H, const int64_t* edge_index, int64_t E, const int64_t* active_eid,
                            int64_t n_active, const float* grad_p, const float* p, const uint32_t* maskbits, float* dz, uint32_t* dvbits,
                            float* feat, sgs_stream_t stream);
int sgs_edge_score_dw2_from_parts(const float* W1, const float* T_raw, const float* U, const float* R_raw, const float* b1, const float* c_raw,
                                  int64_t N, int64_t H, float p_drop, float* dw2, sgs_stream_t stream);
/* ---- Endpoint-dropout scorer: EdgeProbMLP with dropout > 0 (model.py:16-45) ----
 * The reference drops the two endpoint codes of every scored edge independently, x = drop(relu(fcdim(X[src]))), y = drop(relu(fcdim(X[dst]))),
 * before `_edge_score(x, y)`.  relu(fcdim(.)) is row-wise and hoisted to the nodes (A [N, H]); the masks are per (edge, endpoint):
 *   keep_x[e, c] = sgs_dropout_keep(seed_x, site_x, row e, col c),  keep_y likewise,  x_m = A[src e] * keep_x / (1 - p_ep),  y_m = ... .
 * Masked codes differ per edge, so fc1's node-level half U[s] - U[d] does not exist: the kernels contract all 2H features [x_m * y_m | x_m - y_m]
 * against W1 [H, 2H] per edge (fp32 MFMA, LDS-tiled) and never materialise an [E, H] array in the forward.  H % 16 == 0.
 *   sgs_edge_score_epd_fwd       p_out [E]
 *   sgs_edge_score_epd_bwd_core  over the active rows: dv [n, H], hdz_part [cdiv(n, 64), H], dz [n], feat2 [n, 2H] (the features)
 *                                (then d W1 = dv^T feat2 by sgs_gemm_tn, dfeat2 = dv W1 by a library GEMM)
 *   sgs_edge_score_epd_reduce    d A [N, H] from dfeat2 [n, 2H] over both CSR orientations of the active edge list (masks recomputed)
 * ws: sgs_edge_score_epd_workspace_bytes(H). */
/* Probe knobs of the bf16x6 scorer kernels (tools/stagger_probe.py, tools/stagger_trace.py; the product path never calls them).
 * `stagger` >= 0 forces the start-up sleep of every CU's second resident workgroup (in 64-cycle quanta; -1 = the built-in policy),
 * `prio` = 1 runs the main loop at raised wave priority, 2 the epilogue; `mode_mask` = bit m set: kernel MODE m staggers. */
int sgs_edge_score_probe_set(int stagger, int prio, uint32_t mode_mask);
/* `buf` (device, 8 words per workgroup of the next launches, or NULL = off): shader-clock stamps at kernel start, main loop,
 * epilogue and end, and the hardware id of the CU the workgroup ran on. */
int sgs_edge_score_probe_trace(unsigned long long* buf);
size_t sgs_edge_score_epd_workspace_bytes(int64_t H);
int sgs_edge_score_epd_fwd(const float* A, int64_t N, int64_t H, const int64_t* edge_index, int64_t E, int64_t edge_id_offset, const float* W1,
                           const float* b1, const float* w2, const float* b2, float p_hidden, uint64_t seed, uint32_t site, float p_ep,
                           uint64_t seed_x, uint32_t site_x, uint64_t seed_y, uint32_t site_y, float* p_out, void* ws, size_t ws_bytes,
                           sgs_stream_t stream);
int sgs_edge_score_epd_bwd_core(const float* A, int64_t N, int64_t H, const int64_t* edge_index, int64_t E, int64_t edge_id_offset,
                                const int64_t* active_eid, int64_t n_active, const float* grad_p, const float* W1, const float* b1, const float* w2,
                                const float* b2, float p_hidden, uint64_t seed, uint32_t site, float p_ep, uint64_t seed_x, uint32_t site_x,
                                uint64_t seed_y, uint32_t site_y, float* dv, float* hdz_part, float* dz, float* feat2, void* ws, size_t ws_bytes,
                                sgs_stream_t stream);
int sgs_edge_score_epd_reduce(const float* dfeat2, const float* A, int64_t N, int64_t H, const int32_t* in_ptr, const int32_t* in_src,
                              const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                              const int64_t* active_eid, int64_t edge_id_offset, float p_ep, uint64_t seed_x, uint32_t site_x, uint64_t seed_y,
                              uint32_t site_y, float* dA, sgs_stream_t stream);

/* FUSED form of the same backward (round 3), for active rows SORTED BY SOURCE (a drawn subset of a row-sorted edge list, in edge order: every
 * dataset of the reference, datasets.py:189-190 to_undirected emits a coalesced list).  Neither feat nor dfeat exists as an [n, H] array:
 *   sgs_edge_score_bwd_prep_sd        as sgs_edge_score_bwd_prep without feat; sd [n, 2] int32 = the endpoints of every active row
 *   sgs_edge_score_bwd_dfeat_fused    the dfeat contraction with the by-source half of d codes reduced in its epilogue:
 *                                       G [n, H] = dfeat * codes[src]  (for the by-destination half),
 *                                       opart [sgs_edge_score_bwd_fused_opart_rows(n, N), H]: row (r >> 5) + src(r) = the sum of dfeat * codes[dst]
 *                                       over the rows of src(r) inside 32-row tile r >> 5, written by the LAST such row (other rows of opart: undefined)
 *   sgs_gemm_tn_mask_gather           d W1a with feat = codes[src] * codes[dst] gathered per row (gemm_tn section below)
 *   sgs_edge_score_bwd_reduce_fused   d codes[v] = sum of v's opart rows + sum_{in-row v} G;  d U / out_U_raw as sgs_endpoint_reduce_pair_bits
 * Results equal the unfused entry points' up to fp32 summation order.  HBM traffic at n = 100 000, H = 256: ~0.5 GB -> ~0.22 GB. */
int sgs_edge_score_bwd_prep_sd(const float* codes, int64_t N, int64_t H, const int64_t* edge_index, int64_t E, const int64_t* active_eid,
                               int64_t n_active, const float* grad_p, const float* p, const uint32_t* maskbits, float* dz, uint32_t* dvbits,
                               int32_t* sd, sgs_stream_t stream);
size_t sgs_edge_score_bwd_fused_opart_rows(int64_t n, int64_t N);
int sgs_edge_score_bwd_dfeat_fused(const uint32_t* dvbits, const float* dz, const int32_t* sd, const float* codes, int64_t n, int64_t N, int64_t H,
                                   const float* W1, const float* w2, float p_drop, float* G, float* opart, void* ws, size_t ws_bytes,
                                   sgs_stream_t stream);
int sgs_edge_score_bwd_reduce_fused(const float* G, const float* opart, const uint32_t* dvbits, const float* dz, const float* w2, float p_drop,
                                    int64_t N, int64_t H, int64_t nnz, const int32_t* in_ptr, const int32_t* in_eid, const int32_t* out_ptr,
                                    float* out_codes, float* out_U, float* out_U_raw, sgs_stream_t stream);
/* The same chain with the MODE 5 operand packed by the prep launch (one launch fewer; same results, bit for bit):
 *   sgs_edge_score_bwd_prep_sd_pack      sgs_edge_score_bwd_prep_sd + the pack of diag(w2 / (1 - p)) W1a^T into ws
 *                                        (ws_bytes >= sgs_edge_score_workspace_bytes(0, H, 0))
 *   sgs_edge_score_bwd_dfeat_fused_packed  sgs_edge_score_bwd_dfeat_fused on the operand that the prep left in ws (the same ws) */
int sgs_edge_score_bwd_prep_sd_pack(const float* codes, int64_t N, int64_t H, const int64_t* edge_index, int64_t E, const int64_t* active_eid,
                                    int64_t n_active, const float* grad_p, const float* p, const uint32_t* maskbits, float* dz, uint32_t* dvbits,
                                    int32_t* sd, const float* W1, const float* w2, float p_drop, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_dfeat_fused_packed(const uint32_t* dvbits, const float* dz, const int32_t* sd, const float* codes, int64_t n, int64_t N,
                                          int64_t H, float* G, float* opart, const void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_core_bits(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index, int64_t E,
                                 int64_t edge_id_offset, const int64_t* active_eid, int64_t n_active, const float* grad_p, const float* W1,
                                 const float* b1, const float* w2, const float* b2, float p_drop, uint64_t seed, uint32_t site,
                                 uint32_t* dvbits, float* hdz_part, float* dz, float* feat, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_dfeat_bits(const uint32_t* dvbits, const float* dz, int64_t n, int64_t H, const float* W1, const float* w2, float p_drop,
                                  float* dfeat, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_endpoint_reduce_pair_bits(const float* dfeat, const uint32_t* dvbits, const float* dz, const float* w2, float p_drop, const float* codes,
                                  int64_t N, int64_t H, int64_t nnz, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                                  const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* out_codes, float* out_U,
                                  float* out_U_raw, sgs_stream_t stream);
/* C[M, N] (row stride ldc) = (diag(dz) mask diag(rowscale * scale))^T B, mask bits [K, M/32]; colsum_A (optional, [M]) = that matrix's column
 * sums; dz_sum (optional, [1]) = sum_k dz[k] (d fc2.bias rides along); C_raw [M, N] / colsum_raw [M] (optional): the same two results
 * before the factor rowscale * scale (terms of d fc2.weight, sgs_edge_score_dw2_from_parts).  Tall-K shapes only (sgs_gemm_tn_mask_supported);
 * ws: sgs_gemm_tn_workspace_bytes(K, M, N). */
int sgs_gemm_tn_mask_supported(int64_t K, int64_t M, int64_t N);
/* ... with B never materialised: row k of B = codes[src k, :] * codes[dst k, :], (src, dst) = sd[k] (int32 [K, 2]), `codes` [codes_rows, N] row-major (codes_rows * N < 2^32).
 * Bit-identical to sgs_gemm_tn_mask on the materialised rows (same products, same order). */
int sgs_gemm_tn_mask_gather(const uint32_t* Abits, const float* dz, const float* rowscale, float scale, const float* codes, int64_t codes_rows,
                            const int32_t* sd, int64_t K, int64_t M, int64_t N, float* C, int64_t ldc, float* colsum_A, float* dz_sum, float* C_raw,
                            float* colsum_raw, void* ws, size_t ws_bytes, sgs_stream_t stream);
/* A/B switch of sgs_gemm_tn_mask_gather (tests, tools): shared = 1 (default) the shared-operand kernel -- the four waves of a K-group gather,
 * multiply and split a step's rows ONCE and exchange the operand fragments through LDS --, 0 the per-wave-slice kernel of round 2 (also what
 * shapes the shared kernel does not serve fall back to).  slabs > 0 forces the number of K-slices (workgroups per column group). */
void sgs_gemm_tn_set_gather_variant(int shared, int slabs);
int sgs_gemm_tn_mask(const uint32_t* Abits, const float* dz, const float* rowscale, float scale, const float* B, int64_t K, int64_t M, int64_t N,
                     float* C, int64_t ldc, float* colsum_A, float* dz_sum, float* C_raw, float* colsum_raw, void* ws, size_t ws_bytes,
                     sgs_stream_t stream);

/* ---- bf16 mode of the scorer's matrix-core contractions (opt-in; the entries above are the fp32-faithful default and the parity mode).
 * Each entry below has the arguments and outputs of the entry it is named after.  Where that entry issues several bf16 MFMA products per
 * fp32 product over exact operand splits v = v1 + v2 + v3 (v1 = RNE_bf16(v)), these issue ONLY v1 x v1, accumulated in fp32:
 *   forward (MODE 0 unpaired, MODE 3 paired, mask-keeping)  v[e, h] = sum_k bf16(W1a[h, k]) bf16(codes[s, k] * codes[d, k]), then the
 *                                                            unchanged fp32 epilogue (+ U[s] - U[d] + b1, ReLU, dropout, fc2, sigmoid);
 *                                                            a mate's paired score equals the unpaired bf16 score bit for bit
 *   dfeat (mask form, plain / fused / fused_packed)          bf16(diag(w2 / (1 - p)) W1a) against the exact 0 / 1 mask
 *   d W1a (sgs_gemm_tn_mask / _gather)                       bf16(dz[k] * feat[k, :]) against the exact 0 / 1 mask
 * The choice travels with the call (no global state).  H = 128 or 256 (sgs_edge_score_bf16_supported); the GEMM shapes are those of
 * sgs_gemm_tn_mask_supported.  sgs_edge_score_bwd_dfeat_fused_packed_bf16 reads the operand that sgs_edge_score_bwd_prep_sd_pack_bf16 left
 * in ws (the fp32 pair's packed operand is another layout). */
int sgs_edge_score_bf16_supported(int64_t H);
int sgs_edge_score_fwd_bf16(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index, int64_t E,
                            int64_t edge_id_offset, const float* W1, const float* b1, const float* w2, const float* b2, float p_drop,
                            uint64_t seed, uint32_t site, float* p_out, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_fwd_paired_bf16(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index, int64_t E,
                                   int64_t edge_id_offset, const int32_t* canon, int64_t M, const int32_t* mate, const float* W1, const float* b1,
                                   const float* w2, const float* b2, float p_drop, uint64_t seed, uint32_t site, float* p_out, void* ws,
                                   size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_fwd_mask_bf16(const float* codes, const float* U, int64_t N, int64_t H, const int64_t* edge_index, int64_t E,
                                 int64_t edge_id_offset, const int32_t* canon, int64_t M, const int32_t* mate, const float* W1, const float* b1,
                                 const float* w2, const float* b2, float p_drop, uint64_t seed, uint32_t site, float* p_out, uint32_t* maskbits,
                                 void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_dfeat_bits_bf16(const uint32_t* dvbits, const float* dz, int64_t n, int64_t H, const float* W1, const float* w2,
                                       float p_drop, float* dfeat, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_prep_sd_pack_bf16(const float* codes, int64_t N, int64_t H, const int64_t* edge_index, int64_t E, const int64_t* active_eid,
                                         int64_t n_active, const float* grad_p, const float* p, const uint32_t* maskbits, float* dz, uint32_t* dvbits,
                                         int32_t* sd, const float* W1, const float* w2, float p_drop, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_score_bwd_dfeat_fused_bf16(const uint32_t* dvbits, const float* dz, const int32_t* sd, const float* codes, int64_t n, int64_t N,
                                        int64_t H, const float* W1, const float* w2, float p_drop, float* G, float* opart, void* ws, size_t ws_bytes,
                                        sgs_stream_t stream);
int sgs_edge_score_bwd_dfeat_fused_packed_bf16(const uint32_t* dvbits, const float* dz, const int32_t* sd, const float* codes, int64_t n, int64_t N,
                                               int64_t H, float* G, float* opart, const void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_gemm_tn_mask_bf16(const uint32_t* Abits, const float* dz, const float* rowscale, float scale, const float* B, int64_t K, int64_t M, int64_t N,
                          float* C, int64_t ldc, float* colsum_A, float* dz_sum, float* C_raw, float* colsum_raw, void* ws, size_t ws_bytes,
                          sgs_stream_t stream);
int sgs_gemm_tn_mask_gather_bf16(const uint32_t* Abits, const float* dz, const float* rowscale, float scale, const float* codes, int64_t codes_rows,
                                 const int32_t* sd, int64_t K, int64_t M, int64_t N, float* C, int64_t ldc, float* colsum_A, float* dz_sum, float* C_raw,
                                 float* colsum_raw, void* ws, size_t ws_bytes, sgs_stream_t stream);

int sgs_endpoint_reduce(const float* M_out, const float* M_in, const float* T, int64_t N, int64_t H, int64_t nnz,
                        const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, const int32_t* out_ptr,
                        const int32_t* out_dst, const int32_t* out_eid, float sign_out, float sign_in, float* out,
                        sgs_stream_t stream);
/* Both endpoint reductions of the scorer backward in one pass (needs H % 4 == 0, N <= 65536; 16-byte aligned rows):
 *   out_codes = reduce(dfeat, dfeat, T = codes, +1, +1)        out_U = reduce(dv, dv, NULL, +1, -1) */
int sgs_endpoint_reduce_pair(const float* dfeat, const float* dv, const float* codes, int64_t N, int64_t H, int64_t nnz,
                             const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, const int32_t* out_ptr,
                             const int32_t* out_dst, const int32_t* out_eid, float* out_codes, float* out_U, sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K6: gate and losses (training_hybrid.py:92-133, utils.py:163-169, 187-211), all on device.
 * ---------------------------------------------------------------------------------- */
/* correct[0] = #{i in train : argmax_c logits[i,c] == y_i} (first maximum wins), correct[1] = #train.
 * micro-F1 of utils.calculate_f1 == correct[0] / correct[1]; the gate compares two such counts. */
int sgs_masked_correct(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask,
                       int32_t* correct, sgs_stream_t stream);
/* The F1 gate's two counts (learned vs random logits, training_hybrid.py:92-101) in one launch:
 * correct4 = {#correct_a, #train, #correct_b, #train}; correct4 must be ZERO on entry (it is accumulated into). */
int sgs_masked_correct_pair(const float* logits_a, const float* logits_b, int64_t N, int64_t C, const int64_t* y,
                            const uint8_t* train_mask, int32_t* correct4, sgs_stream_t stream);

/* Per-split confusion counts of an evaluation (macro / weighted F1, per-class precision and recall): for every row i and every split s
 * with m_s[i] != 0, conf[s][y_i][argmax_c logits[i, c]] += 1.  conf is int64 [3, C, C] (split, true class, predicted class) and is
 * ACCUMULATED: the call never clears it (the caller zeroes it once per evaluation).  The argmax is sgs_masked_correct's (torch.argmax: the
 * first maximum wins, a row of -inf predicts class 0); NaN logits are out of scope.  A row may be in several masks and is counted in
 * each.  y_i is read only for rows in at least one mask; rows outside every mask may hold any label.  Contract: labels of masked rows
 * lie in [0, C) (a masked row that breaks it is skipped, never used as an index).  Integer atomics only: the result does not depend on
 * arrival order.  One launch, no workspace, no host synchronisation (capturable).  N = 0: SGS_OK, nothing launched; N < 2^32.
 * Two forms: 1 = direct (every C): one wave per row, lane 0 issues up to three non-returning 64-bit global adds;  2 = privatised
 * (12 C^2 <= 65536 bytes, i.e. C <= 73, and N < 2^31): a workgroup of 16 waves keeps an int32 [3, C, C] histogram in LDS over a
 * grid-stride loop (at most one workgroup per CU) and adds its non-zero cells to conf at the end.
 * sgs_confusion_variant(N, C): which form a call launches now (pure host function, needs no GPU): 1 or 2; 0 for N = 0 (nothing); -1 when the
 *   call would return SGS_EINVAL (N < 0, C < 1, or form 2 forced on a shape outside its range).  Automatic rule: 2 iff C <= 12 and
 *   4096 <= N < 2^31, else 1.  Measured ("Per-class evaluation metrics"): the direct form's adds queue up per
 *   128-byte line of conf (3 C^2 / 16 lines), so form 2 wins at few classes and many rows (C = 5: 16.6 against 90.3 us at N = 33 869,
 *   from N = 4096 on; C = 12: 16.1 against 21.2 us) and loses from C = 16 on (C = 41, N = 232 965: 91.1 against 65.1 us).
 * sgs_confusion_variant_set(code): 0 = automatic (default), 1 = direct, 2 = privatised; other codes SGS_EINVAL (the setting is kept).  Forcing 2
 *   makes calls with C > 73 return SGS_EINVAL without a launch.  Read when a call launches; for A/B timing and tests. */
int sgs_confusion_counts(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* m0, const uint8_t* m1, const uint8_t* m2,
                         int64_t* conf, sgs_stream_t stream);
int sgs_confusion_variant(int64_t N, int64_t C);
int sgs_confusion_variant_set(int code);

/* Exact ROC-AUC counts of an evaluation (binary and one-vs-rest), threshold-free and pooled over a loader.
 * Scores are fp32 [N, S], computed by the caller: C = 2 -> S = 1, score = logits[:, 1] - logits[:, 0], an item is positive iff y == 1;
 * C > 2 -> S = C, score = log_softmax(logits, 1), an item of column c is positive iff y == c.  The items of (split s, column c) are the
 * rows with m_s[i] != 0, a label in [0, C) and a non-NaN score.  Order is by float value: -0.0 == +0.0, -inf lowest, +inf highest.  With
 * P, Nn the positive / negative items:  twoU = sum over positive i, negative j of (2 [x_j < x_i] + [x_j == x_i]),  AUC = twoU / (2 P Nn)
 * (undefined when P Nn == 0): sklearn.metrics.roc_auc_score, ties count one half.  twoU is an integer, so every figure here is exact.
 *
 * sgs_auc_block_items(): host only; the number of sorted items one workgroup of the rank-sum kernel owns (tests place tie runs across it).
 * sgs_auc_pack: writes N * S 64-bit keys, keys[i * S + c] =
 *     bits 0-2  the three masks (!= 0 -> 1)          bit 3  positive (y_i == 1 for S = 1, y_i == c otherwise)
 *     bits 4-35 the order-preserving image of the score: -0.0 becomes +0.0, then a negative value has all 32 bits flipped and a
 *               non-negative one its sign bit             bits 36..  the column c
 *   A NaN score clears that item's mask bits; a row whose label is outside [0, C) has the mask bits of all its S items cleared (the label
 *   is compared, never used as an index), so rows outside every mask may hold any label.  Needs (C == 2 and S == 1) or (C > 2 and S == C),
 *   S <= 65536 and N * S < 2^31.  One launch, no workspace, capturable.  N = 0: SGS_OK, nothing launched.
 * sgs_auc_counts: `keys` is any concatenation of packed blocks in any order, n of them; out is int64 [3, S, 3] = {twoU, P, Nn} per
 *   (split, column), WRITTEN (not accumulated).  The call sorts the keys on bits [4, 36 + ceil(log2 S)) into the workspace (the hipCUB
 *   device radix sort: stable, the flag bits ride along; `keys` is not modified) and makes one streaming pass over the sorted keys in tiles of
 *   sgs_auc_block_items(): per-tile negative counts per split, a scan over the tiles, then per tile the inclusive negative prefix, the
 *   tie-run start b and end e of every positive item and its contribution Cn_s(e) + Cn_s(b - 1) (Cn_s: the split's negatives up to a
 *   position, relative to the item's column start; column starts follow from the Nn totals).  A run that reaches a tile edge is closed by
 *   one search in the sorted keys (a bisection done 256 probes at a time by the workgroup) plus one partial-tile count per tile edge,
 *   whatever the run's length.  Integer arithmetic and
 *   integer atomic adds only: the result does not depend on arrival order, and two identical calls give identical bits.  Contract:
 *   every key's column is < S (a key that breaks it is never used as an index; the counts are then unspecified).  Requires n < 2^31 and
 *   S <= 65536, else SGS_EINVAL; n = 0 gives zeros and SGS_OK.
 *   ws: sgs_auc_counts_workspace_bytes(n, S) (host only, needs no GPU).  NOT capturable into a HIP graph: hipCUB clears its counters with
 *   hipMemsetAsync, which must not become a graph node (the reason the sort-path sgs_graph_build is not capturable either); evaluation
 *   is not a captured path. */
int64_t sgs_auc_block_items(void);
int sgs_auc_pack(const float* scores, int64_t N, int64_t S, int64_t C, const int64_t* y, const uint8_t* m0, const uint8_t* m1, const uint8_t* m2,
                 uint64_t* keys, sgs_stream_t stream);
size_t sgs_auc_counts_workspace_bytes(int64_t n, int64_t S);
int sgs_auc_counts(const uint64_t* keys, int64_t n, int64_t S, int64_t* out, void* ws, size_t ws_bytes, sgs_stream_t stream);

/* The gate of training_hybrid.py:95-103 in two launches, no zero fill, no atomics: out5[0..3] = (#correct_a, #train, #correct_b, #train)
 * (argmax of each logit matrix against y on the train rows; lowest index on ties), out5[4] = 0.  With dst_host_mapped (pinned,
 * device-mapped host int32[5]) the finishing launch also hands the four counts to the host as sgs_publish_to_host does (payload, then
 * seq_dev[0] -- or 1 -- as the sequence word with release semantics).  ws: sgs_gate_counts_workspace_bytes(N). */
size_t sgs_gate_counts_workspace_bytes(int64_t N);
int sgs_gate_counts(const float* logits_a, const float* logits_b, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask,
                    int32_t* out5, const uint64_t* seq_dev, int32_t* dst_host_mapped, void* ws, size_t ws_bytes, sgs_stream_t stream);

/* Closing launch of a replayed step: loss_sum[0] += loss[0] and epoch[0] += 1 (either pair may be NULL). */
int sgs_loss_tick(float* loss_sum, const float* loss, uint64_t* epoch, sgs_stream_t stream);
/* Publish n (<= 63) device words to pinned, device-mapped HOST memory: dst[0..n) = src[0..n), then dst[n] = low 32 bits
 * of *seq_dev (NULL: 1) with release semantics at system scope.  A host thread polling dst[n] for a change reads the
 * payload without a copy-engine round trip or a stream synchronisation (the gate read-back of a replayed step). */
int sgs_publish_to_host(const int32_t* src_dev, int64_t n, const uint64_t* seq_dev, int32_t* dst_host_mapped, sgs_stream_t stream);

/* criterion(out[train_mask], y[train_mask]) for criterion = nn.CrossEntropyLoss() (main.py:125;
 * training_hybrid.py:105,139,145): loss[0] = mean over train rows of (logsumexp - logit[y]).
 * row_lse[N], rowloss[N], n_rows[1] are caller scratch kept for backward:
 * dlogits[i,c] = (softmax - onehot) * grad_loss / #train on train rows, 0 elsewhere. */
int sgs_masked_ce_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask,
                      float* loss, float* row_lse, float* rowloss, int32_t* n_rows, sgs_stream_t stream);
int sgs_masked_ce_bwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask,
                      const float* row_lse, const int32_t* n_rows, const float* grad_loss, float* dlogits,
                      sgs_stream_t stream);

/* The two edge regularisers on the q sampled edges (weights w, endpoints sampled_edge_index [2,q]):
 *   reg1 = BCE(w[valid], [y_s == y_d]), valid = both endpoints are train nodes; 0 unless the labels sum
 *          to more than 1 (training_hybrid.py:107-129; the reference's torch.isin + .item() sync)
 *   reg2 = mean_j (w_j - cos(logits[s_j], logits[d_j]))^2           (utils.consistency_loss)
 * out[5] = {reg1, reg2, #valid, sum labels, coef1*reg1 + coef2*reg2}.
 * Backward: dw[q] and per-edge gradient rows Gs, Gd [q,C] wrt logits[src], logits[dst]; the caller
 * folds them into dlogits with sgs_endpoint_reduce(Gs, Gd, NULL, +1, +1) over the sampled graph. */
size_t sgs_edge_reg_workspace_bytes(int64_t q);
int sgs_edge_reg_fwd(const float* w, const int64_t* sampled_edge_index, int64_t q, const float* logits, int64_t N,
                     int64_t C, const int64_t* y, const uint8_t* train_mask, float coef1, float coef2, float* out,
                     float* cos_out, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_edge_reg_bwd(const float* w, const int64_t* sampled_edge_index, int64_t q, int64_t q_global, const float* logits,
                     int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* out, float coef1,
                     float coef2, const float* grad_loss, float* dw, float* Gs, float* Gd, sgs_stream_t stream);

/* The learned branch's whole loss (training_hybrid.py:105-133: criterion + coef1 reg1 + coef2 reg2) in three launches, for
 * criterion = nn.CrossEntropyLoss():  out[7] = {reg1, reg2, #valid, sum labels, coef1 reg1 + coef2 reg2, cross entropy, loss};
 * row_lse[N], rowloss[N], n_rows[1] as sgs_masked_ce_fwd.  Backward: sgs_edge_reg_bwd (reads out[0..4]) -> sgs_endpoint_reduce ->
 * sgs_masked_ce_bwd_acc, which ADDS the cross entropy's gradient to the dlogits already there. */
int sgs_hybrid_loss_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                        const int64_t* sampled_edge_index, int64_t q, float coef1, float coef2, float* out, float* row_lse, float* rowloss,
                        int32_t* n_rows, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_masked_ce_bwd_acc(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* row_lse,
                          const int32_t* n_rows, const float* grad_loss, float* dlogits, sgs_stream_t stream);

/* The same two chains for criterion = nn.CrossEntropyLoss(weight = w, label_smoothing = eps) (reduction "mean", ignore_index -100):
 * F.cross_entropy(logits[train], y[train], weight, label_smoothing).  weight[C] may be NULL (all ones); label_smoothing in [0, 1], 0 skips
 * the smoothing reduction.  With W = sum_c w_c and lse_i = logsumexp_c x_ic:
 *   row_i = (1 - eps) w[y_i] (lse_i - x_i[y_i]) + (eps / C) (W lse_i - sum_c w_c x_ic)   on train rows, 0 elsewhere  (rowloss[N])
 *   den   = sum over train rows of w[y_i]                                                 (den[1], a float: the backward's divisor,
 *                                                                                          in the place n_rows has in the plain chain)
 *   loss  = sum_i row_i / den;  nan when den == 0 (torch forms the hard term's mean on its own: 0 / 0)
 *   dlogits[i,c] = grad_loss / den [ (1 - eps) w[y_i] (softmax_ic - [c == y_i]) + (eps / C) (W softmax_ic - w_c) ] on train rows, 0 elsewhere;
 *                  nan on every train row when den == 0 (as torch)
 * den and W are formed on the device (den from weight, y and the mask in the finishing block; W per workgroup of the backward): no
 * host read-back, no atomics, fixed summation orders.  sgs_masked_ce_w_bwd_acc ADDS to dlogits; sgs_hybrid_loss_w_fwd's out[0..4] are
 * bitwise sgs_hybrid_loss_fwd's (same launches, same order), out[5] is the weighted cross entropy, out[6] = out[5] + out[4].
 * Labels outside [0, C) on train rows are outside the contract (they count with weight 0 here). */
int sgs_masked_ce_w_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                        float label_smoothing, float* loss, float* row_lse, float* rowloss, float* den, sgs_stream_t stream);
int sgs_masked_ce_w_bwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                        float label_smoothing, const float* row_lse, const float* den, const float* grad_loss, float* dlogits,
                        sgs_stream_t stream);
int sgs_masked_ce_w_bwd_acc(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* weight,
                            float label_smoothing, const float* row_lse, const float* den, const float* grad_loss, float* dlogits,
                            sgs_stream_t stream);
int sgs_hybrid_loss_w_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                          const int64_t* sampled_edge_index, int64_t q, float coef1, float coef2, const float* weight, float label_smoothing,
                          float* out, float* row_lse, float* rowloss, float* den, void* ws, size_t ws_bytes, sgs_stream_t stream);

/* The same loss and its gradients in THREE launches, bit for bit the chains above ("Hybrid loss in three launches").
 * `weighted` != 0 selects the weighted / smoothed criterion: norm is then den (a float word), otherwise n_rows (an int32 word) and
 * weight must be NULL, label_smoothing 0.
 *   sgs_hybrid_loss_fused_fwd   one launch for the row losses AND the per-edge terms, then the finishing block of sgs_hybrid_loss_fwd /
 *                               _w_fwd: out[7], row_lse[N], rowloss[N], norm[1] as there.  stash [q, 4] floats, 16-byte aligned, NULL
 *                               when no gradient is wanted: per sampled edge {1 / sqrt(max(|x|^2 |y|^2, 1e-16)), cos / |x|^2, cos / |y|^2
 *                               (both 0 under the clamp), 2 (w - cos) coef2 / q} -- what the backward needs of the three dot products.
 *   sgs_hybrid_loss_fused_bwd   one launch over the sampled graph's two CSR orientations (nnz = q; the traversal sgs_endpoint_reduce
 *                               takes for (q, N)): dlogits[N, C] = the regularisers' gradient, formed per entry from stash and two
 *                               logits rows (no [q, C] arrays), plus the cross entropy's on train rows; dw[q] as sgs_edge_reg_bwd.
 *                               Both outputs are written, not accumulated.  Meant for coef2 != 0 (with coef2 == 0 the stash's last
 *                               word is 0 and dlogits gets -0 * ... terms where the chain above writes the cross entropy alone). */
int sgs_hybrid_loss_fused_fwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w,
                              const int64_t* sampled_edge_index, int64_t q, float coef1, float coef2, int weighted, const float* weight,
                              float label_smoothing, float* out, float* row_lse, float* rowloss, void* norm, float* stash, void* ws,
                              size_t ws_bytes, sgs_stream_t stream);
int sgs_hybrid_loss_fused_bwd(const float* logits, int64_t N, int64_t C, const int64_t* y, const uint8_t* train_mask, const float* w, int64_t q,
                              const float* stash, const float* out, float coef1, int weighted, const float* weight, float label_smoothing,
                              const float* row_lse, const void* norm, const float* grad_loss, const int32_t* in_ptr, const int32_t* in_src,
                              const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* dw,
                              float* dlogits, sgs_stream_t stream);

/* Edge-sharded losses: raw[4] ={sum bce, sum (w-cos)^2, #valid, sum labels} over THIS rank's sampled edges; the
 * ranks all-reduce raw, form reg1 / reg2 with the global q, and call sgs_edge_reg_bwd with out[2], out[3] = the
 * global #valid / label sum and q_global = the global number of sampled edges (q_global = q when unsharded). */
int sgs_edge_reg_partial(const float* w, const int64_t* sampled_edge_index, int64_t q, const float* logits, int64_t N,
                         int64_t C, const int64_t* y, const uint8_t* train_mask, float* raw, void* ws, size_t ws_bytes,
                         sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K8: GAT attention (PyG 2.3.1 GATConv, heads = 1; model.py:189-208 via torch_geometric's GAT):
 *   e_k = leaky_relu(a_src[src_k] + a_dst[dst_k], slope) over each node's in-edges + one self loop
 *   (existing (i,i) edges are ignored, as PyG removes them), soft = softmax per destination
 *   (denominator + 1e-16), alpha = dropout(soft, p) keyed by (seed, site, edge id) / (site+1, node).
 * sgs_gat_alpha_fwd writes soft/alpha in dst-CSR entry order (+ per-node loop values); the aggregation
 * out = sum_k alpha_k x'[src_k] + alpha_loop x'[i] + bias is sgs_spmm_csr(val = alpha_in, diag =
 * alpha_loop); backward: galpha (per edge id) / gloop from sgs_sddmm_csr, then sgs_gat_alpha_bwd gives
 * g_edge[eid] = dL/d(a_src[src]+a_dst[dst]) per edge, g_selfloop[i], and d_a_dst[i]; d_a_src is the
 * per-source sum of g_edge (sgs_spmm_csr over the src-CSR with D = 1) + g_selfloop.
 * sgs_gather_by_eid / sgs_scatter_by_eid re-order per-edge arrays between edge-id and CSR entry order.
 * ---------------------------------------------------------------------------------- */
/* Node-level attention scores of a GATConv layer in one pass over x' [N, D]: a_src[i] = <x'[i, :], att_src>, a_dst likewise (GATConv's
 * (x' * att).sum(-1)); backward: dxl (+)= g_src (x) att_src + g_dst (x) att_dst (accumulate != 0: added to dxl), d att_src = sum_i g_src[i] x'[i, :],
 * d att_dst likewise (fixed summation order).  ws: sgs_gat_scores_bwd_workspace_bytes(N, D). */
int sgs_gat_scores_fwd(const float* xl, int64_t N, int64_t D, const float* att_src, const float* att_dst, float* a_src, float* a_dst,
                       sgs_stream_t stream);
size_t sgs_gat_scores_bwd_workspace_bytes(int64_t N, int64_t D);
int sgs_gat_scores_bwd(const float* xl, int64_t N, int64_t D, const float* att_src, const float* att_dst, const float* g_src, const float* g_dst,
                       int accumulate, float* dxl, float* datt_src, float* datt_dst, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_gat_alpha_fwd(const float* a_src, const float* a_dst, int64_t N, int64_t n_edges, const int32_t* in_ptr,
                      const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed,
                      uint32_t site, float* soft_in, float* soft_loop, float* alpha_in, float* alpha_loop,
                      sgs_stream_t stream);
int sgs_gat_alpha_bwd(const float* a_src, const float* a_dst, int64_t N, int64_t n_edges, const int32_t* in_ptr,
                      const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed,
                      uint32_t site, const float* soft_in, const float* soft_loop, const float* galpha,
                      const float* gloop, float* g_edge, float* g_selfloop, float* d_a_dst, sgs_stream_t stream);
int sgs_gather_by_eid(const float* by_eid, const int32_t* eid, int64_t n, float* out_order, sgs_stream_t stream);
int sgs_scatter_by_eid(const float* in_order, const int32_t* eid, int64_t n, float* by_eid, sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K8h: multi-head GATConv (PyG 2.3.1 semantics restated, 1 <= K <= 16 heads of C >= 1 channels; K = 1 callers keep the entry points
 * above).  x' = lin_src(x) is [N, K C] with head-major columns (x'[i, h, c] at column h C + c), att_* are [K, C] flat.
 * Layout: per-node arrays are [N, K]; per-edge arrays (soft, alpha, galpha, g_edge) are EDGE-MAJOR [n_edges, K], indexed by EDGE ID
 * (v[eid * K + h]; a row's K values contiguous), so the dst-CSR and the src-CSR kernels read one array through their eid columns and
 * no re-ordering launch exists.  Each kernel reads an entry's CSR indices once for all K heads.  No float atomics: every sum runs in
 * CSR order over a fixed shuffle tree (run-to-run identical).  No host synchronisation, scratch from the caller: capturable.
 * Any other (K, C) returns SGS_EINVAL with a message; sgs_gat_heads_supported is the host-only predicate (no GPU needed).
 *   forward : sgs_gat_scores_heads_fwd -> sgs_gat_alpha_heads_fwd -> sgs_spmm_csr_heads (in-CSR; mode CONCAT or MEAN)
 *   backward: sgs_spmm_csr_heads over the out-CSR (d x'), sgs_sddmm_csr_heads (galpha, gloop), sgs_gat_alpha_heads_bwd,
 *             sgs_edge_sum_by_row_heads over the out-CSR (d a_src), sgs_gat_scores_heads_bwd
 * Attention dropout is keyed (seed, site, row = edge id, col = head) for edges and (site + 1, row = node, col = head) for the loops:
 * sgs_dropout_keep(seed, site, n_edges, K, p) / (seed, site + 1, N, K, p) export exactly the masks used, and column 0 at K = 1 is
 * sgs_gat_alpha_fwd's mask.
 * ---------------------------------------------------------------------------------- */
#define SGS_HEADS_CONCAT 0    /* X [N, K C] -> Y [N, K C], per-head weights */
#define SGS_HEADS_MEAN 1      /* X [N, K C] -> Y [N, C] = mean over heads (GATConv concat = False), fused into the aggregation */
#define SGS_HEADS_BROADCAST 2 /* X [N, C] shared by the heads -> Y [N, K C] / K: the transposed aggregation behind MEAN's backward */
int sgs_gat_heads_supported(int64_t K, int64_t C);
/* Which kernel instantiation and launch shape an entry point of this section picks (a pure host function; the launchers decode ITS
 * result, so the two cannot drift).  op: SGS_GAT_OP_* below; aligned16 != 0: every pointer the entry point tests is 16-byte aligned
 * (scores fwd: xl, att_src, att_dst; SpMM: X, Y; SDDMM: A, B; ignored by the others, as is C by SGS_GAT_OP_ROW and N by all but
 * SGS_GAT_OP_SCORES_BWD).  -1: unsupported (K, C), N < 0 or unknown op.
 *   code = kind * 1000000 + VEC * 100000 + lg * 10000 + lgG * 1000 + W
 *   kind  1 gat_scores_heads_fwd       VEC floats per lane and load, 2^lg lanes per (node, head) unit
 *         2 gat_scores_heads_bwd       W = rows per workgroup (16 | 64 at N >= 4096 | 256 at N >= 65536) (+ gat_scores_bwd_finish)
 *         3 spmm_csr_heads CONCAT      VEC, 2^lg lanes per row (256 >> lg rows per workgroup)
 *         4 spmm_csr_heads_mean_lds    MEAN at K C <= 1024: VEC, 2^lg lanes per row over the K C per-head columns
 *         5 spmm_csr_heads_mean        MEAN at K C > 1024: VEC, 2^lg lanes per row over the C output columns, each walking the heads
 *         6 spmm_csr_heads BROADCAST   as kind 3
 *         7 sddmm_csr_heads            VEC, 2^lg lanes per row = KP 2^lgG: 2^lgG lanes per head, KP = 2^(lg - lgG) head slots
 *         8 sddmm_csr_heads broadcast  as kind 7
 *         9 the per-row family         W = KP = K rounded up to a power of two (64 / KP entries per step); VEC 1
 *   VEC = 4 needs C % 4 == 0 and the alignment; lg <= 6. */
#define SGS_GAT_OP_SCORES_FWD 0      /* sgs_gat_scores_heads_fwd */
#define SGS_GAT_OP_SCORES_BWD 1      /* sgs_gat_scores_heads_bwd */
#define SGS_GAT_OP_SPMM_CONCAT 2     /* sgs_spmm_csr_heads, mode SGS_HEADS_CONCAT */
#define SGS_GAT_OP_SPMM_MEAN 3       /* ... SGS_HEADS_MEAN */
#define SGS_GAT_OP_SPMM_BROADCAST 4  /* ... SGS_HEADS_BROADCAST */
#define SGS_GAT_OP_SDDMM 5           /* sgs_sddmm_csr_heads, broadcast == 0 */
#define SGS_GAT_OP_SDDMM_BROADCAST 6 /* ... broadcast != 0 */
#define SGS_GAT_OP_ROW 7             /* sgs_gat_alpha_heads_fwd / _bwd, sgs_gat_alpha_heads_edge_fwd / _bwd, sgs_edge_sum_by_row_heads */
int sgs_gat_heads_variant(int op, int64_t N, int64_t K, int64_t C, int aligned16);
/* a_src[i, h] = <x'[i, h, :], att_src[h, :]>, a_dst likewise, one pass over x'.  Backward as sgs_gat_scores_bwd with g_src / g_dst [N, K]
 * and d att_* [K, C]; ws: sgs_gat_scores_heads_bwd_workspace_bytes(N, K, C). */
int sgs_gat_scores_heads_fwd(const float* xl, int64_t N, int64_t K, int64_t C, const float* att_src, const float* att_dst, float* a_src,
                             float* a_dst, sgs_stream_t stream);
size_t sgs_gat_scores_heads_bwd_workspace_bytes(int64_t N, int64_t K, int64_t C);
int sgs_gat_scores_heads_bwd(const float* xl, int64_t N, int64_t K, int64_t C, const float* att_src, const float* att_dst, const float* g_src,
                             const float* g_dst, int accumulate, float* dxl, float* datt_src, float* datt_dst, void* ws, size_t ws_bytes,
                             sgs_stream_t stream);
/* Segment softmax (+ attention dropout) per (destination, head) over the dst-CSR and its backward; formulas of sgs_gat_alpha_fwd / _bwd.
 * soft / alpha / galpha / g_edge [n_edges, K] by edge id ((i, i) entries get 0), *_loop / g_selfloop / d_a_dst [N, K]. */
int sgs_gat_alpha_heads_fwd(const float* a_src, const float* a_dst, int64_t N, int64_t K, int64_t n_edges, const int32_t* in_ptr,
                            const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site,
                            float* soft, float* soft_loop, float* alpha, float* alpha_loop, sgs_stream_t stream);
int sgs_gat_alpha_heads_bwd(const float* a_src, const float* a_dst, int64_t N, int64_t K, int64_t n_edges, const int32_t* in_ptr,
                            const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site,
                            const float* soft, const float* soft_loop, const float* galpha, const float* gloop, float* g_edge, float* g_selfloop,
                            float* d_a_dst, sgs_stream_t stream);
/* The same softmax with an edge term (PyG 2.3.1 GATConv(edge_dim = 1), edge_attr = the edge weight, restated): with edge_w [n_edges] by
 * edge id and edge_coef [K] (c_h = <lin_edge.weight[h, :], att_edge[h, :]>, computed by the caller) the logit of edge e = (s -> i) is
 * leaky_relu(a_src[s, h] + a_dst[i, h] + edge_w[e] c_h); (i, i) entries are removed, entries of weight 0 stay, and the added loop of
 * node i carries wbar_i = the mean weight of i's remaining in-edges (fill_value = 'mean'; 0 without any).  Everything after the logit
 * (softmax, dropout sites and keys, outputs) is sgs_gat_alpha_heads_fwd's; 1 <= K <= 16, K = 1 included.  The forward also writes
 * loop_w [N] = wbar and loop_inv_cnt [N] = 1 / cnt_i (0 without in-edges) from the row walk it makes anyway; the backward reads them.
 * Backward: g_edge / g_selfloop / d_a_dst as sgs_gat_alpha_heads_bwd, and
 *   d_edge_w[e]    = sum_h c_h (g_edge[e, h] + g_selfloop[i, h] / cnt_i) (+ dw_add[e] unless NULL: a second layer's gradient, summed on
 *                    the way out), 0 for (i, i) entries;
 *   d_edge_coef[h] = sum_e edge_w[e] g_edge[e, h] + sum_i wbar_i g_selfloop[i, h]: per-workgroup partials in ws
 *                    (sgs_gat_alpha_heads_edge_bwd_workspace_bytes(N, K)), added in a fixed order by a second small launch.
 * No float atomics, no host synchronisation. */
int sgs_gat_alpha_heads_edge_fwd(const float* a_src, const float* a_dst, const float* edge_w, const float* edge_coef, int64_t N, int64_t K,
                                 int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, float negative_slope,
                                 float p_drop, uint64_t seed, uint32_t site, float* soft, float* soft_loop, float* alpha, float* alpha_loop,
                                 float* loop_w, float* loop_inv_cnt, sgs_stream_t stream);
size_t sgs_gat_alpha_heads_edge_bwd_workspace_bytes(int64_t N, int64_t K);
int sgs_gat_alpha_heads_edge_bwd(const float* a_src, const float* a_dst, const float* edge_w, const float* edge_coef, const float* loop_w,
                                 const float* loop_inv_cnt, int64_t N, int64_t K, int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src,
                                 const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site, const float* soft,
                                 const float* soft_loop, const float* galpha, const float* gloop, const float* dw_add, float* g_edge,
                                 float* g_selfloop, float* d_a_dst, float* d_edge_w, float* d_edge_coef, void* ws, size_t ws_bytes,
                                 sgs_stream_t stream);
/* out[j, h] = sum over row j of the CSR (ptr, eid) of g_edge[eid_k, h] (+ g_self[j, h] unless NULL), in CSR order: d a_src over the out-CSR. */
int sgs_edge_sum_by_row_heads(const float* g_edge, const float* g_self, int64_t N, int64_t K, int64_t nnz, const int32_t* ptr, const int32_t* eid,
                              float* out, sgs_stream_t stream);
/* Per-head SpMM: Y[i, h C + c] = sum_k val[eid_k, h] X[col_k, h C + c] + diag[i, h] X[i, h C + c] (diag may be NULL), then bias / act /
 * dropout exactly as sgs_spmm_csr (bias over Y's columns; dropout keyed (site, row i, Y column)).  mode: SGS_HEADS_*.  Rows are 16-byte
 * vectorised when C % 4 == 0 (a lane's columns then belong to one head); any other C runs column by column. */
int sgs_spmm_csr_heads(const float* X, int64_t N, int64_t K, int64_t C, int64_t nnz, const int32_t* ptr, const int32_t* col, const int32_t* eid,
                       const float* val, const float* diag, int mode, const float* bias, int act, float p_drop, uint64_t seed, uint32_t site,
                       float* Y, sgs_stream_t stream);
/* Per-head SDDMM: g[eid_k, h] = <A[i, h, :], B[col_k, h, :]> for k in row i, gdiag[i, h] = <A[i, h, :], B[i, h, :]>; A, B [N, K C].
 * broadcast != 0: A is [N, C], shared by the heads, and the products are scaled by 1 / K (backward of SGS_HEADS_MEAN). */
int sgs_sddmm_csr_heads(const float* A, const float* B, int64_t N, int64_t K, int64_t C, int64_t nnz, const int32_t* ptr, const int32_t* col,
                        const int32_t* eid, int broadcast, float* g, float* gdiag, sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K8c: GATv2 attention (PyG 2.3.1 GATv2Conv, share_weights = False, restated; csrc/gatv2.hip).  xl = lin_l(x), xr = lin_r(x) [N, K C]
 * (head-major columns), att [K, C]; for an entry j -> i, head h:
 *   s[c] = xl[j, h, c] + xr[i, h, c] (+ edge_w[e] lin_edge[h, c]),   logit = sum_c att[h, c] leaky_relu(s[c]).
 * Softmax per (destination, head) over the in-entries plus one added loop, / (sum + 1e-16); existing (i, i) entries are removed (their
 * soft / alpha / g_logit / d_edge_w are 0); attention dropout sites and keys are sgs_gat_alpha_heads_fwd's.  edge_w == NULL: no edge
 * term (lin_edge, loop_w, loop_inv_cnt and their gradients are then ignored and may be NULL).  With it, edge_w [n_edges] by edge id,
 * lin_edge [K, C] = lin_edge.weight, the loop of node i carries wbar_i = the mean weight of i's remaining in-edges (0 without any), and
 * the forward writes loop_w [N] = wbar, loop_inv_cnt [N] = 1 / cnt_i (0 without in-edges) for the backward.  1 <= K <= 16, any C >= 1;
 * rows are 16-byte vectorised when C % 4 == 0 and the pointers are 16-byte aligned.  Aggregation and the d alpha SDDMM are
 * sgs_spmm_csr_heads / sgs_sddmm_csr_heads.  Backward, with galpha / gloop from the SDDMM:
 *   sgs_gatv2_alpha_heads_bwd (dst-CSR): g_logit [n_edges, K] by edge id, g_loop [N, K] (the logits' gradients), and with
 *       t[c] = g att[h, c] leaky_relu'(s[c]):  d_xr[i] = sum t over i's entries and loop;  d_att[h, c] = sum g leaky_relu(s[c]);
 *       d_lin_edge[h, c] = sum t w;  d_edge_w[e] = sum_{h, c} t lin_edge[h, c] + the loop's own such sum / cnt_i (+ dw_add[e] unless
 *       NULL: a second layer's gradient, summed on the way out).  d_att / d_lin_edge: per-workgroup partials in ws
 *       (sgs_gatv2_alpha_heads_bwd_workspace_bytes(N, K, C)), added in a fixed order by a second small launch.
 *   sgs_gatv2_dxl_heads (src-CSR): d_xl[j] (+)= sum over j's out-entries and loop of t, recomputed from g_logit / g_loop;
 *       accumulate != 0 adds onto d_xl's contents (the aggregation's d xl).
 * No float atomics, no host synchronisation: two identical launches give identical bits.
 *   sgs_gatv2_alpha_heads_fwd_multi (batched ensemble evaluation, forward only, no attention dropout): sgs_gatv2_alpha_heads_fwd with
 *       p_drop = 0 for all D draws of a pass in ONE launch (draw = blockIdx.y) over sgs_graph_filter_multi's draw-strided dst-CSRs:
 *       in_ptr [D, N+1], in_src / in_eid [D, max(nnz, 1)].  Draw d reads xl / xr + d * x_stride (in floats), the shared att [K C], and --
 *       with the edge term -- edge_w [D, max(nnz, 1)] by the DRAW's edge id (what in_eid holds: sgs_sample_topq_multi's st_weights) with
 *       the shared lin_edge [K C]; edge_w == NULL: no edge term (lin_edge ignored).  It writes block d of alpha [D, max(nnz, 1), K] by the
 *       draw's edge id and of alpha_loop [D, N, K].  Eval needs neither soft / soft_loop copies nor loop_w / loop_inv_cnt: none are taken,
 *       none are written; the raw logits wait in `alpha` itself between the kernel's two sweeps (each lane re-reads only what it wrote).
 *       Block d is BITWISE what sgs_gatv2_alpha_heads_fwd writes to alpha / alpha_loop for draw d's arrays with p_drop = 0, with and
 *       without the edge term: both kernels instantiate one row-walk body (the same pre-activation, trip order, online max / sum,
 *       shuffle order, 1 / (sum + 1e-16), zeros for drawn (i, i) entries), and the launch is sgs_gatv2_variant(SGS_GATV2_OP_ALPHA_FWD, N,
 *       K, C, aligned16) of the base pointers, as the single-draw launcher chooses it.
 *       x_stride is 0 (one [N, K C] pair shared by all draws: layer 1) or EXACTLY N K C (dense per-draw blocks: layer 2); every other
 *       value is SGS_EINVAL.  Reason: the vector width (float4 or scalar) changes which channels a lane sums and so the bits of a logit.
 *       With these two strides every draw's block has the base pointer's 16-byte alignment whenever C % 4 == 0, so block d takes the
 *       variant a single-draw call on that block takes; a padded stride could not promise that.
 *       Requires 0 <= N, nnz < 2^31, 1 <= D <= 65535, 1 <= K <= 16, C >= 1 ("bad sizes"); edge_w needs lin_edge; N = 0 returns SGS_OK with
 *       nothing launched.  No workspace, no atomics, no memset nodes, no host synchronisation: capturable.
 *
 * sgs_gatv2_variant: which kernel instantiation and lane geometry an entry point launches, as a pure host function (the three launchers
 * and sgs_gatv2_alpha_heads_bwd_workspace_bytes decode its result, so the two cannot drift).  op: SGS_GATV2_OP_* below; aligned16 != 0:
 * every pointer the entry point accesses by vectors is 16-byte aligned (forward: xl, xr, att, and lin_edge with edge_w; backward: those
 * and d_xr; dxl: those and d_xl).  -1: unsupported (K, C), N < 0 or unknown op.
 *   code = kind * 1000000 + VEC * 100000 + lg * 10000 + lgG * 1000 + ONE * 100 + iters
 *   kind  1 gatv2_alpha_heads_fwd   2^lg = KP 2^lgG lanes per row (KP = K rounded up to a power of two, 2^lgG <= 64 / KP lanes per head,
 *                                   256 >> lg rows per workgroup), VEC floats per lane and chunk of 2^lgG VEC channels; ONE = 1: a head's
 *                                   C channels fit one chunk (C <= VEC 2^lgG) and stay in registers; iters = 0
 *         2 gatv2_alpha_heads_bwd   the same geometry; iters = row passes per workgroup = passes / 2048 clamped to 1 .. 16 with
 *                                   passes = ceil(N / (256 >> lg)); ceil(passes / iters) workgroups (+ gatv2_param_finish)
 *         3 gatv2_dxl_heads         2^lg lanes per row over the K C / VEC column groups; lgG = ONE = iters = 0
 *   VEC = 4 needs C % 4 == 0 and the alignment; lg <= 6.
 * ---------------------------------------------------------------------------------- */
#define SGS_GATV2_OP_ALPHA_FWD 0 /* sgs_gatv2_alpha_heads_fwd */
#define SGS_GATV2_OP_ALPHA_BWD 1 /* sgs_gatv2_alpha_heads_bwd */
#define SGS_GATV2_OP_DXL 2       /* sgs_gatv2_dxl_heads */
int sgs_gatv2_variant(int op, int64_t N, int64_t K, int64_t C, int aligned16);
int sgs_gatv2_alpha_heads_fwd(const float* xl, const float* xr, const float* att, const float* edge_w, const float* lin_edge, int64_t N,
                              int64_t K, int64_t C, int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                              float negative_slope, float p_drop, uint64_t seed, uint32_t site, float* soft, float* soft_loop, float* alpha,
                              float* alpha_loop, float* loop_w, float* loop_inv_cnt, sgs_stream_t stream);
int sgs_gatv2_alpha_heads_fwd_multi(const float* xl, const float* xr, int64_t x_stride, const float* att, const float* edge_w,
                                    const float* lin_edge, int64_t N, int64_t K, int64_t C, int64_t D, int64_t nnz, const int32_t* in_ptr,
                                    const int32_t* in_src, const int32_t* in_eid, float negative_slope, float* alpha, float* alpha_loop,
                                    sgs_stream_t stream);
size_t sgs_gatv2_alpha_heads_bwd_workspace_bytes(int64_t N, int64_t K, int64_t C);
int sgs_gatv2_alpha_heads_bwd(const float* xl, const float* xr, const float* att, const float* edge_w, const float* lin_edge, const float* loop_w,
                              const float* loop_inv_cnt, int64_t N, int64_t K, int64_t C, int64_t n_edges, const int32_t* in_ptr,
                              const int32_t* in_src, const int32_t* in_eid, float negative_slope, float p_drop, uint64_t seed, uint32_t site,
                              const float* soft, const float* soft_loop, const float* galpha, const float* gloop, const float* dw_add,
                              float* g_logit, float* g_loop, float* d_xr, float* d_att, float* d_lin_edge, float* d_edge_w, void* ws,
                              size_t ws_bytes, sgs_stream_t stream);
int sgs_gatv2_dxl_heads(const float* xl, const float* xr, const float* att, const float* edge_w, const float* lin_edge, const float* loop_w,
                        const float* g_logit, const float* g_loop, int64_t N, int64_t K, int64_t C, int64_t nnz, const int32_t* out_ptr,
                        const int32_t* out_dst, const int32_t* out_eid, float negative_slope, int accumulate, float* d_xl,
                        sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K8d: GINE aggregation (PyG 2.3.1 GINEConv, edge_dim = 1 with the edge weight as the attribute, restated; csrc/gine.hip).  x [N, D],
 * a = lin.weight[:, 0] and b = lin.bias [D] (lin = Linear(1, D)), edge_w [n_edges] by edge id or NULL (unit weights: w = 1.0f in the
 * same expressions, bitwise the result of a vector of ones), diag = 1 + eps:
 *   z[i, c] = diag x[i, c] + sum_{e: j -> i} relu(x[j, c] + (edge_w[e] a[c] + b[c]))
 * (i, i) and duplicate entries are ordinary entries.  Any D >= 1; N = 0, n_edges = 0 and empty rows are fine.  Rows are gathered 16 / 8
 * bytes at a time when D % 4 / D % 2 == 0 and x, z / dz, d_x, a, b are aligned to that, else column by column; one wave per row, or a
 * workgroup of 4 / 16 waves per row for few long rows (sgs_gine_variant: kind * 1000 + VEC * 100 + W, a pure host function).
 *   sgs_gine_aggregate_fwd (dst-CSR: in_ptr / in_src / in_eid) writes z.  It stores no mask.
 *   sgs_gine_aggregate_bwd (src-CSR: out_ptr / out_dst / out_eid), with m = dz[dst_e, c] where x[j, c] + (edge_w[e] a[c] + b[c]) > 0, else 0:
 *       d_x[j, c]   = diag dz[j, c] + sum_{e: j -> .} m          (d_x == NULL: not computed, nothing written)
 *       d_edge_w[e] = sum_c a[c] m (+ dw_add[e] unless NULL: another layer's gradient, summed on the way out)   (NULL: not computed)
 *       d_a[c] = sum_e edge_w[e] m,  d_b[c] = sum_e m             (both NULL: not computed; else per-workgroup partials in ws,
 *                                                                 sgs_gine_aggregate_bwd_workspace_bytes(N, D), added in a fixed order by
 *                                                                 a second small launch; N = 0 writes zeros)
 * Mask-recompute contract: the backward evaluates the pre-activation with the same explicit expression as the forward, x + (w a + b), on
 * the same fp32 inputs, and the library is compiled with -ffp-contract=off (no fused multiply-add on either side): the two agree bit
 * for bit, so an element passes the ReLU in the backward iff it did in the forward.
 * No float atomics, no memset nodes, no host synchronisation: two identical launches give identical bits.
 *   sgs_gine_aggregate_fwd_multi (batched ensemble evaluation, forward only): sgs_gine_aggregate_fwd for all D draws of a pass in ONE
 *       launch (draw = blockIdx.y) over sgs_graph_filter_multi's draw-strided dst-CSRs: in_ptr [D, N+1], in_src / in_eid [D, max(nnz, 1)].
 *       Draw d reads x + d * x_stride (in floats; 0: one [N, Dc] block shared by all draws; else >= N Dc: per-draw blocks), edge_w
 *       [D, max(nnz, 1)] by the DRAW's edge id (what in_eid holds: sgs_sample_topq_multi's st_weights) or NULL (unit weights, bitwise a
 *       vector of ones), the shared a, b [Dc], and writes block d of z [D, N, Dc].  Block d is BITWISE sgs_gine_aggregate_fwd on draw d's
 *       arrays: the same device code per workgroup (the same gather body and pre-activation expression), the row form chosen by
 *       sgs_gine_variant(N, Dc, nnz, .) as a single-draw call with n_edges = nnz chooses it.  VEC decides which lane owns a column, never
 *       the order of a column's additions, so it may differ from the single-draw call's without changing a bit; here it is the widest
 *       that x, z, a, b AND the strides between draws (x_stride, N Dc) allow -- an unaligned stride drops to a narrower VEC.
 *       Requires N >= 0, Dc >= 1, nnz >= 0, 1 <= D <= 65535, x_stride == 0 or >= N Dc ("bad sizes"); x and z must not overlap; N = 0
 *       returns SGS_OK with nothing launched.  No workspace, no atomics, no memset nodes, no host synchronisation: capturable.
 * ---------------------------------------------------------------------------------- */
int sgs_gine_variant(int64_t N, int64_t D, int64_t nnz, int align_bytes);
int sgs_gine_aggregate_fwd(const float* x, const float* edge_w, const float* a, const float* b, float diag, int64_t N, int64_t D,
                           int64_t n_edges, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, float* z,
                           sgs_stream_t stream);
int sgs_gine_aggregate_fwd_multi(const float* x, int64_t x_stride, const float* edge_w, const float* a, const float* b, float diag,
                                 int64_t N, int64_t Dc, int64_t nnz, int64_t D, const int32_t* in_ptr, const int32_t* in_src,
                                 const int32_t* in_eid, float* z, sgs_stream_t stream);
size_t sgs_gine_aggregate_bwd_workspace_bytes(int64_t N, int64_t D);
int sgs_gine_aggregate_bwd(const float* x, const float* dz, const float* edge_w, const float* a, const float* b, float diag, int64_t N,
                           int64_t D, int64_t n_edges, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                           const float* dw_add, float* d_x, float* d_edge_w, float* d_a, float* d_b, void* ws, size_t ws_bytes,
                           sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K9: Chebyshev layers of order K > 1 (PyG 2.3.1 ChebConv, normalization = 'sym', lambda_max = 2, restated; 1 <= K <= 8 -- the bound is
 * a choice, not a hardware limit; K = 1 callers need none of this, the layer is a Linear).  For edges (s_e -> d_e) with weights w_e:
 *   (i, i) edges are removed (weight 0 in every formula, gradient 0);  deg_n = sum_{e: s_e = n} w_e, summed BY SOURCE (not the GCN
 *   degree);  dis = deg^-1/2 (inf -> 0);  l_e = -dis[s_e] w_e dis[d_e]: the off-diagonal entries of L_hat = 2 L / lambda_max - I, whose
 *   diagonal is 0 (no loop term);  (L_hat X)_i = sum_{e: d_e = i} l_e X[s_e] (duplicates count twice).
 * Nothing assumes a symmetric edge list.  No float atomics (row sums in CSR order over a fixed tree: run-to-run identical), no host
 * synchronisation, scratch from the caller: capturable.  An order outside 1..8 returns SGS_EINVAL ("unsupported ...");
 * sgs_cheb_supported is the host-only predicate (no GPU needed).
 *   sgs_cheb_norm_fwd : dis [N], l_in / l_out [n_edges] = l in dst-CSR / src-CSR entry order (bitwise equal copies); w == NULL = unit weights.
 *   sgs_cheb_norm_bwd : g [n_edges] = dLoss/dl by EDGE ID -> dw [n_edges]:  dw_e = -dis[s] dis[d] g_e + c[s_e] with
 *                       c_n = -1/2 dis_n^3 (sum_{e: s_e = n} -w_e dis[d_e] g_e + sum_{e: d_e = n} -dis[s_e] w_e g_e), and dw_e = 0 on (i, i)
 *                       edges.  g2 (may be NULL): a second layer's gradient over the same normalisation, summed on read.
 *                       ws: sgs_cheb_norm_bwd_workspace_bytes(N).
 *   sgs_cheb_spmm     : one step of the three-term recurrence,
 *                         Y[i, :] = act(add[i, :] + alpha * sum_{k in row i} val[k] X[col[k], :] - sub[i, :] + bias)
 *                       over D columns.  K is the layer's order and is only validated here (the step itself does not depend on it): this
 *                       is the entry point through which an unsupported order reports "unsupported".  X, add, sub, Y have their OWN leading dimensions (ld* >= D), so the steps of Clenshaw's recurrence
 *                       b_k = Y_k + 2 L_hat b_{k+1} - b_{k+2} and of its backward U_k = 2 L_hat^T U_{k-1} - U_{k-2} read and write column
 *                       blocks of the concatenated [N, K D] buffers in place.  add, sub, bias may be NULL; add may be Y itself; X must
 *                       not overlap Y or Y2.  Y2 (may be NULL): a second copy scale2 * Y with leading dimension ldy2 (the backward
 *                       writes 2 U_k straight into the SDDMM's operand).  act / p_drop / seed / site as sgs_spmm_csr: the mask is
 *                       sgs_dropout_keep(seed, site, row i, column c).  The forward runs over (in_ptr, in_src, l_in), the backward over
 *                       (out_ptr, out_dst, l_out); nnz picks the row-per-workgroup kernel as in sgs_spmm_csr.  Rows are gathered 16 bytes
 *                       at a time when D % 4 == 0, ldx % 4 == 0 and X is 16-byte aligned, else column by column.
 *   sgs_cheb_spmm_variant : which kernel sgs_cheb_spmm launches for a shape (a pure host function, no GPU needed; the launchers switch on
 *                       it), in sgs_spmm_csr_variant's encoding: VEC * 100 + LPR for a group of LPR lanes per row, 1000 + VEC * 100 + NW
 *                       for a workgroup of NW waves per row (N <= 65536 and nnz >= 16 N; NW = 16 from nnz >= 256 N).  aligned16 is about X
 *                       alone.  0 for N == 0 or D == 0 (no launch), -1 for negative sizes.
 * The gradient wrt l is ONE sgs_sddmm_csr at width (K - 1) D of [G | 2 U_1 | ... | 2 U_{K-2}] against [b_1 | ... | b_{K-1}].
 * ---------------------------------------------------------------------------------- */
int sgs_cheb_supported(int64_t K);
int sgs_cheb_norm_fwd(const float* w, int64_t n_edges, int64_t N, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                      const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* dis, float* l_in, float* l_out,
                      sgs_stream_t stream);
size_t sgs_cheb_norm_bwd_workspace_bytes(int64_t N);
int sgs_cheb_norm_bwd(const float* w, const float* g, const float* g2, int64_t n_edges, int64_t N, const float* dis, const int32_t* in_ptr,
                      const int32_t* in_src, const int32_t* in_eid, const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                      const int64_t* edge_index, float* dw, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_cheb_spmm_variant(int64_t N, int64_t D, int64_t nnz, int64_t ldx, int aligned16);
int sgs_cheb_spmm(int64_t K, const float* X, int64_t ldx, int64_t N, int64_t D, int64_t nnz, const int32_t* ptr, const int32_t* col,
                  const float* val, float alpha, const float* add, int64_t ldadd, const float* sub, int64_t ldsub, const float* bias, int act,
                  float p_drop, uint64_t seed, uint32_t site, float* Y, int64_t ldy, float* Y2, int64_t ldy2, float scale2,
                  sgs_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Weight-gradient GEMM of the node-level Linear layers: C[M,N] = A^T B, A [K,M], B [K,N] row-major,
 * K = number of graph nodes (dW = dY^T X for GCNConv.lin, model.py:94-95,151-153).  fp32 MFMA fed from
 * coalesced global reads, split-K with a fixed-order combine (deterministic).  Skinny shapes only (the
 * vendor GEMM serves the rest): meant for M, N <= ~1k.  K >= 8192 (with M % 4 == 0, N % 2 == 0) takes a tall-K kernel:
 * 128 x 64 output tile and a K-slice per wave, one 16-B + one 8-B load per 8 MFMAs (dW1a = dv^T feat, K = q rows).
 * ---------------------------------------------------------------------------------- */
size_t sgs_gemm_tn_workspace_bytes(int64_t K, int64_t M, int64_t N);
int sgs_gemm_tn(const float* A, const float* B, int64_t K, int64_t M, int64_t N, float* C, void* ws, size_t ws_bytes,
                sgs_stream_t stream);
/* Same product with the column sums of A as a by-product (colsum_A [M]; d b1 = colsum(dv) of the scorer's backward rides
 * on d W1a = dv^T feat): only for the shapes the tall-K kernel serves with a split -- ask sgs_gemm_tn_can_colsum first. */
void sgs_gemm_tn_set_tall_variant(int variant);   /* tall-K shapes (K >= 8192): 1 / -1 = bf16x6 kernel (default; fp32-faithful, see sgs_edge_score_set_variant), 0 = fp32-MFMA kernel */
int sgs_gemm_tn_can_colsum(int64_t K, int64_t M, int64_t N);
int sgs_gemm_tn_colsum(const float* A, const float* B, int64_t K, int64_t M, int64_t N, float* C, float* colsum_A, void* ws,
                       size_t ws_bytes, sgs_stream_t stream);
/* The same product written with row stride ldc >= N, i.e. into a column block of a wider matrix: the two halves of d fc1.weight
 * [H, 2H] (model.py:29-31: W1 [x*y | x-y]) are d W1a = dv^T feat and d W1b = dU^T codes, each an [H, H] block with ldc = 2H.
 * colsum_A may be NULL (otherwise as sgs_gemm_tn_colsum).  Workspace: sgs_gemm_tn_workspace_bytes(K, M, N). */
int sgs_gemm_tn_ld(const float* A, const float* B, int64_t K, int64_t M, int64_t N, float* C, int64_t ldc, float* colsum_A, void* ws,
                   size_t ws_bytes, sgs_stream_t stream);
/* Several independent products in one call: the weight gradients of a training step are leaves of its backward (only the optimiser
 * reads them), each a latency-bound launch of a few dozen workgroups at partition size.  The problems whose shape takes the
 * partition-sized kernel (one workgroup per 32 x 32 tile of C, its waves the K-slices; sgs_gemm_tn_group_supported > 0) share ONE
 * launch per workgroup size, up to eight problems each, over the sum of their tiles; every other problem goes through sgs_gemm_tn_ld
 * in list order (and needs its `ws`; the grouped ones do not read it).  Every C is bit-identical to the single call's.  The
 * problems must be independent: no C may overlap an operand or another C.  ldc = 0 means N.
 * sgs_gemm_tn_group_supported: the waves per workgroup (2, 4, 8 or 16) the partition-sized kernel runs this shape with, 0 when the
 * shape takes another kernel -- the single call and the grouped one both decide by it. */
typedef struct SgsGemmTnProblem {
    const float* A;        /* [K, M] */
    const float* B;        /* [K, N] */
    int64_t K, M, N;
    float* C;              /* [M, N], row stride ldc */
    int64_t ldc;
    void* ws;              /* sgs_gemm_tn_workspace_bytes(K, M, N); may be NULL when sgs_gemm_tn_group_supported(K, M, N) > 0 */
    size_t ws_bytes;
} SgsGemmTnProblem;
int sgs_gemm_tn_group_supported(int64_t K, int64_t M, int64_t N);
int sgs_gemm_tn_group(const SgsGemmTnProblem* problems, int count, sgs_stream_t stream);

/* ----------------------------------------------------------------------------------
 * Effective-resistance edge prior (datasets.py:159-173 add_ER; estimator: EffectiveResistanceWeights.ipynb cell 11 er_edge).
 * weight[e] = max(0, sum_{i < walk_lengths} (X_is/deg s - X_it/deg t - Y_is/deg s + Y_it/deg t) / walks) with X / Y the
 * numbers of `walks` uniform random walks of length i from s / t that end at s or t (reference: walk_lengths = 4, walks = 100).
 * out_ptr / out_dst: CSR of the symmetric, coalesced edge list (sgs_graph_build); counter-based randomness keyed on
 * (seed, edge, walk, step).  The host applies softmax(weight * E^-1/2) as add_ER does.
 * ---------------------------------------------------------------------------------- */
int sgs_er_weight(const int64_t* edge_index, int64_t E, int64_t N, const int32_t* out_ptr, const int32_t* out_dst, int walk_lengths,
                  int walks, uint64_t seed, float* weight, sgs_stream_t stream);

/* ----------------------------------------------------------------------------------
 * Optimiser (training_hybrid.py:22-27, 135-141: two torch.optim.Adam steps per batch).
 * One launch updates up to sgs_adam_max_tensors() tensors with torch.optim.Adam's rule (coupled weight decay, no amsgrad):
 *   desc_host [n_tensors][7] int64 in HOST memory, read during the call only (the descriptors travel by value in the
 *             kernel arguments): {param, grad, exp_avg, exp_avg_sq, numel, step, gate}; the pointers are DEVICE addresses;
 *             `step` is that tensor's float counter of completed steps (one per parameter, as torch), read and then
 *             incremented by the kernel, so the call is capturable into a HIP graph; `gate` is 0 or the address of a
 *             device float: while it reads 0 the tensor (and its counter) is left untouched (data-parallel training: the
 *             scorer's tensors are skipped on steps where no rank took the learned branch, decided without a host round trip)
 *   ticket    device uint32, zero on first use (the kernel leaves it zero); one per concurrently running call
 * ---------------------------------------------------------------------------------- */
int sgs_adam_max_tensors(void);
int sgs_adam_step(const int64_t* desc_host, int64_t n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int maximize, uint32_t* ticket, sgs_stream_t stream);
/* Several optimisers' steps in ONE launch, plus the step's closing bookkeeping (round 3).  training_hybrid.py:136-137 steps
 * optimizer_edge_prob and then optimizer_gnn; the two overlap on edge_prob_mlp.gcn* (main.py:100-109, 122), so those tensors are updated
 * twice with the same gradient.  A descriptor names a tensor once and carries one or two optimiser states, applied in order:
 *   desc_host  [n_tensors][11] int64: {param, grad, numel, exp_avg, exp_avg_sq, step, gate, exp_avg2, exp_avg_sq2, step2, gate2}
 *              (exp_avg2 == 0: one state; gates as in sgs_adam_step)
 *   hyper_host [n_tensors][12] float: {lr, beta1, beta2, eps, weight_decay, maximize} of the first state, then of the second
 * loss_sum / loss / epoch (each pair optional): the last workgroup also does what sgs_loss_tick does.  n_tensors <= sgs_adam_multi_max_tensors(). */
int sgs_adam_multi_max_tensors(void);
int sgs_adam_step_multi(const int64_t* desc_host, const float* hyper_host, int64_t n_tensors, uint32_t* ticket, float* loss_sum, const float* loss,
                        uint64_t* epoch, sgs_stream_t stream);

/* ---------------------------------------------------------------- batched ensemble evaluation (evaluate.py:70-173)
 * All D draws of one partition in one pass.  Forward only (no autograd state), for the GCN, GAT and GIN heads.
 *
 * sgs_sample_topq_multi: D draws of sgs_sample_topq over ONE candidate set.  Draw d uses stream id stream_id0 + d (or noise row d of
 *   noise [D, E]) and is bitwise what sgs_sample_topq returns for it (small- and large-E path, ties to the lowest edge id).  Modes as
 *   sgs_sample_topq (LEARNED with or without prior, PRIOR, p == NULL uniform).  The normaliser is reduced once; every radix-select stage
 *   is one launch for all draws (draw index in the grid).  Outputs: mask [D, E] u8, sampled_eid [D, q] (ascending), optional
 *   sampled_edge_index [D, 2, q], stats [D, 4] (optional unless st_weights), optional st_weights [D, q] (sgs_st_weights_fwd's values,
 *   mode LEARNED).  1 <= D <= 65535.  Not available under sgs_dyn_edges_set.
 * sgs_sample_topq_multi_cover: D draws of sgs_sample_topq_cover over ONE candidate set (the node-covering rule described at that entry
 *   point).  Arguments as sgs_sample_topq_multi plus N, in_ptr [N + 1], in_src / in_eid [E] (the destination-row CSR of the candidate
 *   graph, as sgs_sample_topq_cover takes it) and cover_info [D, 2] int32 (may be NULL) = {M_d, min(M_d, q)} per draw.  Row d of mask,
 *   sampled_eid, sampled_edge_index, stats, st_weights and cover_info is bitwise what sgs_sample_topq_cover (followed by
 *   sgs_st_weights_fwd) returns for stream id stream_id0 + d or noise row d, on the small- and the large-E path: stats[d][2] is the
 *   threshold with the flag bit cleared, stats[d][3] the ties taken at the boosted threshold.  Launches: sgs_sample_topq_multi's plus TWO
 *   for all draws.  After the key pass one draw-grouped forced-edge kernel (grid: row blocks x ceil(D / G)) walks the CSR once per group
 *   of G draws: a lane reads an entry (in_src[j], in_eid[j]) once, gathers that edge's key from each of the group's stored key rows
 *   (G independent gathers in flight), keeps one 64-bit (key bits << 32 | ~edge id) maximum per draw, sets bit 31 of each draw's winner
 *   in that draw's key row and moves its count in that draw's top-digit histogram from bin b to bin b + 1024 (integer atomics, first
 *   aggregated per workgroup and draw in LDS).  Lanes per row (sgs_sample_topq_cover_variant), the hand-over of long rows to the whole
 *   workgroup and the bounds checks are the single-draw kernel's.  Before the straight-through weights one finishing launch
 *   (blockIdx.y = draw) writes cover_info and takes the flag bit off the reported thresholds.  q == 0 / q == E: M depends on neither keys
 *   nor draw, so the single-draw key-less count runs once and every row of cover_info gets the same pair.  E == 0 returns at once and
 *   writes nothing.  All counting is integer: results do not depend on G or the launch geometry.  Refused under sgs_dyn_edges_set;
 *   1 <= D <= 65535, E < 2^31 and N < 2^31.  Workspace: sgs_sample_topq_multi's plus 1024 counts per draw.
 *   sgs_sample_topq_multi_cover_group_set(G): draws per workgroup of the grouped kernel, 1, 2 or 4, or 0 for the built-in default
 *   (process-wide).  A measurement hook (tools/eval_cover_ab.py): results are bitwise the same for every G.
 * sgs_graph_filter_multi: the in-CSR + loop_eid of each draw's subgraph (D masks / sampled_eid over the parent's cached in-CSR); every
 *   draw's arrays equal sgs_graph_filter's.  in_ptr [D, N+1], in_src / in_eid [D, q], loop_eid [D, N].  No out-CSR.
 * sgs_gcn_norm_fwd_multi: sgs_gcn_norm_fwd's in-direction outputs per draw (dis, loopw, what_loop [D, N], what_in [D, q]); w [D, q] or
 *   NULL (unit weights).  Same device code: bitwise equal per draw.
 * sgs_spmm_csr_multi: Y[d] = act(A_d X_d + bias) over the per-draw CSRs (ptr [D, N+1], col / val [D, nnz], diag [D, N] or NULL);
 *   X_d = X + d * x_stride (0: one X shared by all draws); Y [D, N, Dc]; act NONE or RELU.  Equal per draw to sgs_spmm_csr.
 * sgs_ensemble_mean_correct: running fp32 sum of Dc logit blocks (logits + d * x_stride, [N, C] each; x_stride 0 = the same block Dc
 *   times) into acc [N, C] (first: acc starts from block 0; else from acc), in draw order.  last: acc *= 1/D_total when D_total > 1,
 *   then argmax (first maximum wins) against y on mask0..2 accumulated into counts [6] int64 = {correct, total} x 3 (not cleared).
 * sgs_gat_alpha_fwd_multi: sgs_gat_alpha_fwd without attention dropout (p = 0, no soft_* outputs) over each draw's in-CSR (in_ptr
 *   [D, N+1], in_src [D, nnz] from sgs_graph_filter_multi): draw d reads a_src + d * a_stride, a_dst + d * a_stride (0: node scores
 *   shared by all draws; N: [D, N] blocks) and writes alpha_in [D, nnz] (0 at (i,i) entries), alpha_loop [D, N].  Same device code:
 *   row d is bitwise sgs_gat_alpha_fwd's.  1 <= D <= 65535.
 * The per-head GAT kernels and the Chebyshev step have the same draw-strided forms (forward only, no attention dropout, no kept softmax,
 * no out-CSR; blockIdx.y = draw; an operand is addressed as base + d * stride, stride 0 = shared by all draws):
 * sgs_gat_alpha_heads_fwd_multi: sgs_gat_alpha_heads_fwd (edge_coef NULL) or sgs_gat_alpha_heads_edge_fwd (edge_w [D, nnz] by the draw's
 *   edge id, edge_coef [K]; every 1 <= K <= 16) at p = 0 over each draw's in-CSR (in_ptr [D, N+1], in_src / in_eid [D, nnz]); node
 *   scores a_src / a_dst + d * a_stride (0: one [N, K] pair; N K: [D, N, K] blocks); alpha [D, nnz, K] by the draw's edge id,
 *   alpha_loop [D, N, K].  The device code of a row is the single-draw kernel's: row d is bitwise its alpha / alpha_loop.
 * sgs_spmm_csr_heads_multi: sgs_spmm_csr_heads, mode CONCAT (Y [D, N, K C]) or MEAN (Y [D, N, C]; the LDS form when a workgroup's rows fit
 *   4096 floats, else lanes walk the heads: the single-draw choice), val [D, nnz, K], diag [D, N, K] or NULL, X + d * x_stride (0: shared);
 *   bias / ReLU epilogue (act NONE or RELU).  Block d is bitwise sgs_spmm_csr_heads' for draw d.
 * sgs_cheb_norm_fwd_multi: dis [D, N] and l_in [D, q] (dst-CSR entry order of each draw) of sgs_cheb_norm_fwd for w [D, q] by the draw's
 *   edge id (NULL: unit weights).  The degree is summed by source without an out-CSR of the draws: the PARENT's out-CSR (pout_*) is walked
 *   under draw d's mask [D, E_parent] with the weights scattered to [D, E_parent] by parent edge id (sampled_eid [D, q]; ws:
 *   sgs_cheb_norm_fwd_multi_workspace_bytes(E_parent, D)), the selected entries handed to the lanes that own them in the filtered out-row,
 *   so every partial sum adds the same values in the same order: dis and l_in are bitwise the single-draw results.
 * sgs_cheb_spmm_multi: one sgs_cheb_spmm step for all draws, Y_d[i, :] = act(add_d[i, :] + alpha * sum_k val_d[k] X_d[col_d[k], :] -
 *   sub_d[i, :] + bias); X, add, sub, Y keep their own leading dimensions and have their own draw strides (0: shared; Y's must give every
 *   draw a block of its own); ptr [D, N+1], col / val [D, nnz]; act NONE or RELU, no Y2.  The row form (nnz per draw) and the vector width
 *   follow sgs_cheb_spmm's rules: block d is bitwise that call's result. */
size_t sgs_sample_topq_multi_workspace_bytes(int64_t E, int64_t D);
int sgs_sample_topq_multi(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise, uint64_t seed,
                          uint64_t stream_id0, int64_t D, int64_t E, int64_t q, const int64_t* edge_index, uint8_t* mask, int64_t* sampled_eid,
                          int64_t* sampled_edge_index, float* stats, float* st_weights, void* ws, size_t ws_bytes, sgs_stream_t stream);
size_t sgs_sample_topq_multi_cover_workspace_bytes(int64_t E, int64_t N, int64_t D);
int sgs_sample_topq_multi_cover_group_set(int G);
int sgs_sample_topq_multi_cover(int mode, const float* p, const float* prior, double degree_bias_coef, const float* noise, uint64_t seed,
                                uint64_t stream_id0, int64_t D, int64_t E, int64_t q, const int64_t* edge_index, int64_t N,
                                const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid, uint8_t* mask, int64_t* sampled_eid,
                                int64_t* sampled_edge_index, float* stats, float* st_weights, int32_t* cover_info, void* ws, size_t ws_bytes,
                                sgs_stream_t stream);
size_t sgs_graph_filter_multi_workspace_bytes(int64_t E_parent, int64_t N, int64_t D);
int sgs_graph_filter_multi(const int32_t* pin_ptr, const int32_t* pin_src, const int32_t* pin_eid, int64_t E_parent, int64_t N, int64_t D,
                           const uint8_t* mask, const int64_t* sampled_eid, int64_t q, int32_t* in_ptr, int32_t* in_src, int32_t* in_eid,
                           int32_t* loop_eid, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_gcn_norm_fwd_multi(const float* w, int64_t q, int64_t N, int64_t D, const int32_t* in_ptr, const int32_t* in_src, const int32_t* in_eid,
                           const int32_t* loop_eid, float* dis, float* loopw, float* what_in, float* what_loop, sgs_stream_t stream);
int sgs_spmm_csr_multi(const float* X, int64_t x_stride, int64_t N, int64_t Dc, int64_t nnz, int64_t D, const int32_t* ptr, const int32_t* col,
                       const float* val, const float* diag, const float* bias, int act, float* Y, sgs_stream_t stream);
int sgs_gat_alpha_fwd_multi(const float* a_src, const float* a_dst, int64_t a_stride, int64_t N, int64_t D, int64_t nnz,
                            const int32_t* in_ptr, const int32_t* in_src, float negative_slope, float* alpha_in, float* alpha_loop,
                            sgs_stream_t stream);
int sgs_gat_alpha_heads_fwd_multi(const float* a_src, const float* a_dst, int64_t a_stride, const float* edge_w, const float* edge_coef,
                                  int64_t N, int64_t K, int64_t D, int64_t nnz, const int32_t* in_ptr, const int32_t* in_src,
                                  const int32_t* in_eid, float negative_slope, float* alpha, float* alpha_loop, sgs_stream_t stream);
int sgs_spmm_csr_heads_multi(const float* X, int64_t x_stride, int64_t N, int64_t K, int64_t C, int64_t nnz, int64_t D, const int32_t* ptr,
                             const int32_t* col, const int32_t* eid, const float* val, const float* diag, int mode, const float* bias, int act,
                             float* Y, sgs_stream_t stream);
size_t sgs_cheb_norm_fwd_multi_workspace_bytes(int64_t E_parent, int64_t D);
int sgs_cheb_norm_fwd_multi(const float* w, const int64_t* sampled_eid, const uint8_t* mask, int64_t q, int64_t N, int64_t E_parent, int64_t D,
                            const int32_t* pout_ptr, const int32_t* pout_dst, const int32_t* pout_eid, const int32_t* in_ptr,
                            const int32_t* in_src, const int32_t* in_eid, float* dis, float* l_in, void* ws, size_t ws_bytes,
                            sgs_stream_t stream);
int sgs_cheb_spmm_multi(int64_t K, const float* X, int64_t ldx, int64_t x_stride, int64_t N, int64_t D, int64_t nnz, int64_t n_draws,
                        const int32_t* ptr, const int32_t* col, const float* val, float alpha, const float* add, int64_t ldadd,
                        int64_t add_stride, const float* sub, int64_t ldsub, int64_t sub_stride, const float* bias, int act, float* Y, int64_t ldy,
                        int64_t y_stride, sgs_stream_t stream);
int sgs_ensemble_mean_correct(const float* logits, int64_t x_stride, int64_t Dc, int64_t N, int64_t C, float* acc, int first, int last,
                              int64_t D_total, const int64_t* y, const uint8_t* mask0, const uint8_t* mask1, const uint8_t* mask2, int64_t* counts,
                              sgs_stream_t stream);

/* ---------------------------------------------------------------- sparsifier export: consensus of D draws (sparsify.py)
 * The fixed sparse graph a trained sparsifier is deployed with: every candidate edge is counted over D draws, and the q edges drawn
 * most often -- ties broken by the score -- are kept.  All counting is integer and every result is independent of arrival order and of
 * the launch geometry.  No call allocates, synchronises or reads back; zero fills are kernels.
 *
 * sgs_consensus_accum: count[e] = (first ? 0 : count[e]) + #{d < Dc : mask[d * mask_stride + e] != 0} for e < E.  `mask` is a pass's
 *   [Dc, E] block of sgs_sample_topq_multi (any non-zero byte counts once; mask_stride >= E in bytes, any alignment).  A thread keeps 16
 *   edges' counts as packed bytes and reads each row through the aligned 16-byte granules that hold its bytes; a granule that is not wholly
 *   inside the block [mask, mask + (Dc - 1) mask_stride + E) is read byte by byte, so no byte outside the block is touched.  `hist` (may be
 *   NULL): int64 [128], ACCUMULATED, never cleared: after this pass's addition hist[count[e]] += 1 for every e (privatised in LDS per
 *   workgroup, non-zero bins flushed with 64-bit adds).  0 <= Dc <= 127 (a count stays below 128 as long as the caller folds at most 127
 *   draws in total; a larger stored count breaks the contract and lands in bin 127).  E = 0: SGS_OK, nothing launched.  Dc = 0: SGS_OK; with
 *   `first` the counts are still zeroed.  E < 2^32.
 * sgs_consensus_select: key_e = (uint32(count_e) << 25) | (bits(p_e) >> 6), the low part 0 when p == NULL or when !(p_e >= 0) (negative,
 *   -0, NaN); a count outside [0, 127] breaks the contract and is clamped, never used as an index.  The q largest keys are selected, ties to
 *   the lowest edge id, by sgs_sample_topq's radix select, count and stable compaction (the fused small-E path up to 2 M edges, the large-E
 *   path above; the key pass fuses the first digit's histogram) and emitted in ORIGINAL edge order: mask [E] u8, eid [q] ascending,
 *   edge_index_out [2, q] (needs edge_index [2, E]), count_out [q] (the clamped counts), p_out [q] = p[eid] (1 when p == NULL), keys_out [E]
 *   (tests).  Every output but mask may be NULL.  The key is a pure integer function of its inputs.  SCORES THAT DIFFER ONLY IN THEIR 6 LOWEST
 *   MANTISSA BITS TIE (and go to the lower edge id): the price of a 32-bit key for the existing select.  q == 0 selects nothing, q == E
 *   everything; q > E returns SGS_EINVAL.  E = 0: SGS_OK.  ws: sgs_consensus_select_workspace_bytes(E), 256-B aligned.  The call takes its
 *   sizes as given (it ignores sgs_dyn_edges_set).
 * sgs_edge_class_counts: pairs[y[src_e]][y[dst_e]] += 1 for every e < n with mask == NULL or mask[e] != 0.  pairs is int64 [C, C],
 *   ACCUMULATED (the caller zeroes it); edge_index is [2, n] with row stride n.  An edge with an endpoint outside [0, N) or a label outside
 *   [0, C) is skipped, never used as an index.  Two forms, chosen by capability alone: 2 = privatised (an int32 [C, C] table in LDS per
 *   workgroup over a grid-stride loop, non-zero cells flushed at the end) when 4 C^2 <= 65536 bytes (C <= 128) and n < 2^31; 1 = direct
 *   (one 64-bit global add per edge) otherwise.  With few classes nearly every edge of a homophilous graph hits one of C diagonal cells,
 *   hence the privatised default.  n = 0: SGS_OK, nothing launched.
 * sgs_edge_class_variant(n, C): the form a call launches now (pure host function): 2 or 1; 0 for n = 0; -1 when the call would return
 *   SGS_EINVAL (n < 0, C < 1, or form 2 forced outside its range).
 * sgs_edge_class_variant_set(code): 0 = automatic (default), 1 = direct, 2 = privatised; other codes SGS_EINVAL.  For tests and A/B timing. */
int sgs_consensus_accum(const uint8_t* mask, int64_t mask_stride, int64_t Dc, int64_t E, int first, int32_t* count, int64_t* hist,
                        sgs_stream_t stream);
size_t sgs_consensus_select_workspace_bytes(int64_t E);
int sgs_consensus_select(const int32_t* count, const float* p, int64_t E, int64_t q, const int64_t* edge_index, uint8_t* mask, int64_t* eid,
                         int64_t* edge_index_out, int32_t* count_out, float* p_out, uint32_t* keys_out, void* ws, size_t ws_bytes,
                         sgs_stream_t stream);
int sgs_edge_class_counts(const int64_t* edge_index, int64_t n, const uint8_t* mask, const int64_t* y, int64_t N, int64_t C, int64_t* pairs,
                          sgs_stream_t stream);
int sgs_edge_class_variant(int64_t n, int64_t C);
int sgs_edge_class_variant_set(int code);

/* ---- device partitioner (partition.py: partition_graph; csrc/partition.hip; numpy restatement: tests/partition_ref.py)
 * One sweep of a balanced k-way label propagation is sgs_lp_propose followed by sgs_lp_commit; all of it is integer arithmetic, so the
 * results are exact and the same on every call.  The graph is an int32 CSR (ptr [N + 1], col [nnz]) of an undirected graph stored both ways;
 * entries with col == row are ignored, repeated entries count with their multiplicity.  part is int32 [N] with values in [0, P) or -1
 * (unassigned); 1 <= P <= min(N, 4096); N, nnz < 2^31.  A column outside [0, N) or a part outside [0, P) is skipped, never used as an index.
 * sgs_lp_propose: for every ELIGIBLE node v (eligible = 0: part[v] == -1; eligible = 1: fmix32(v ^ fmix32(hash_key)) & 1, fmix32 = murmur3's
 *   32-bit finaliser) with conn[p] = the number of non-loop entries u of row v with part[u] = p >= 0, own = conn[part[v]] (0 when unassigned):
 *   best[v] = the p != part[v] with the largest conn[p] > 0 (ties: the lower p), gain[v] = conn[best] - own -- if such a p exists and
 *   gain >= mingain; best[v] = -1, gain[v] = 0 otherwise and for every node that is not eligible.  One wave per row, a slab of P counters in
 *   LDS per wave; a row of more than sgs_lp_propose_hub_row() entries is walked by its workgroup's four waves together (one kernel, both
 *   forms in it).  No float arithmetic, no global atomics.
 * sgs_lp_commit: with size [P] and part as they stand on entry, key(v) = best << 51 | (2^20 - 1 - clamp(gain, 0, 2^20 - 1)) << 31 | v:
 *   within each target, in ascending key order, the first max(cap - size[target], 0) proposals survive; among the survivors with a source
 *   part s >= 0, ordered by the same key with s in place of best, the first max(size[s] - lo, 0) per source survive; survivors without a
 *   source always pass.  Survivors move: part and size are updated in place and *moved (a device int32) is SET to their number.  Two library
 *   radix sorts (csrc/graph_sort.hip), so the call is not capturable into a HIP graph.  ws: sgs_lp_commit_workspace_bytes(N, P) (host only).
 * sgs_partition_stats: size[p] = #{v: part[v] = p} (int32 [P]) and *cut (device int64) = the number of stored non-loop entries (v, u) with
 *   part[v] != part[u] -- every undirected edge twice -- in one pass; both outputs are overwritten.
 * Argument errors (SGS_EINVAL, message in sgs_last_error): N or nnz negative or >= 2^31; P outside [1, 4096]; P > N; a null pointer. */
int64_t sgs_lp_propose_hub_row(void);
int sgs_lp_propose(const int32_t* ptr, const int32_t* col, int64_t N, int64_t nnz, int64_t P, const int32_t* part, int eligible, uint32_t hash_key,
                   int mingain, int32_t* best, int32_t* gain, sgs_stream_t stream);
size_t sgs_lp_commit_workspace_bytes(int64_t N, int64_t P);
int sgs_lp_commit(const int32_t* best, const int32_t* gain, int64_t N, int64_t P, int64_t cap, int64_t lo, int32_t* part, int32_t* size,
                  int32_t* moved, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_partition_stats(const int32_t* ptr, const int32_t* col, int64_t N, int64_t nnz, int64_t P, const int32_t* part, int32_t* size,
                        int64_t* cut, sgs_stream_t stream);

/* ---- neighbour-sampled batches (data.py: ResidentGraph, NeighborLoader; csrc/neighbor.hip; numpy restatement: tests/neighbor_ref.py)
 * A batch is a set of distinct seed nodes plus a sampled k-hop in-neighbourhood.  The graph is the edge list sorted by (src, dst) (int64
 * [2, E]; an edge's id is its position), its two int32 CSRs as sgs_graph_build emits them (rows in ascending edge id) and N nodes; N, E < 2^31.
 * All of it is integer arithmetic: results are exact and the same on every call.  A row id, an edge id or a column outside its range is
 * skipped and never used as an index -- with one exception that indexes nothing: sgs_nbr_select passes the ids of a row through unread.
 * sgs_nbr_select: for frontier row r (node rows[r]; deg = its in-CSR row length, 0 when the node is outside [0, N)) writes take = deg
 *   (fanout = -1 or deg <= fanout) or take = fanout ids to chosen[offs[r] .. offs[r] + take), offs = the exclusive scan of take over the rows
 *   (kept in ws; from in_ptr alone).  Of a longer row the ids e with the `fanout` smallest keys fmix32(e ^ key) are taken (fmix32 = murmur3's
 *   32-bit finaliser, a bijection: distinct ids never tie), in row order.  *total_dev (may be NULL) = offs[n_rows]; nothing is written at or
 *   beyond chosen[cap].  One wave per row: four 8-bit radix passes over a 256-bin LDS histogram, keys recomputed, then a ballot compaction; a
 *   row of more than sgs_nbr_select_hub_row() entries is walked by its workgroup's four waves together (one kernel, both forms in it).  Two
 *   launches (scan, rows).  ws: sgs_nbr_select_workspace_bytes(n_rows), 8-byte aligned.
 * sgs_nbr_select_weighted: the same contract, workspace and two launches, with a weighted draw.  in_wq: int32 [nnz] in in-CSR order (entry j is
 *   the weight of edge in_eid[j]), a quantised weight in [0, 2^24 - 1] (read as unsigned; a larger value counts as 2^24 - 1).  The key of id e is
 *   sgs_nbr_weighted_key(fmix32(e ^ key), wq): with x = max(hash, 1) and NL = 32 * 2^24 - LOG2Q(x) in [1, 2^29] (-log2 of a uniform variate in
 *   24-bit fixed point), LOG2Q(NL) - LOG2Q(wq) + 24 * 2^24 < 2^30 for wq >= 1, and 2^32 - 1 for wq = 0.  Its order is that of -ln(u) / w, so the
 *   `fanout` smallest keys are `fanout` successive draws proportional to the weight, without replacement.  LOG2Q(x), 1 <= x < 2^32: n =
 *   floor(log2 x), m = the 32 bits below the leading one, i = m >> 24, r = (m >> 8) & 0xFFFF, (n << 24) + T[i] + (((T[i + 1] - T[i]) r) >> 16),
 *   T[i] = floor(2^24 log2(1 + i / 256)) (sgs_nbr_log2_table writes the 257 words; built by integer squaring at compile time); within
 *   [-2.9e-6, 0] of log2 x and monotone.  Keys can tie: a longer row takes every id with a key below the fanout-th smallest key t and then the
 *   first fanout - #{key < t} ids with key == t in row order; so zero-weight ids are taken only when a row has fewer than `fanout` positive
 *   ones, first come first.  A row still emits min(fanout, deg) ids.  Only the ratios of the weights inside one row matter.  The row forms are
 *   sgs_nbr_select's; a one-wave row computes its keys in the first radix pass and keeps them in LDS (32 KiB per workgroup, plus 1 KiB for the
 *   table), a row above sgs_nbr_select_hub_row() recomputes them in every pass.  Both pins run on the host (no device needed) and are the
 *   function the kernel evaluates.
 * state: sgs_nbr_state_bytes(N) bytes, 4-byte aligned: three bitmaps of ceil(N / 32) words -- batch members, reached this hop, seeds.
 * sgs_nbr_begin: clears the state and sets the seeds in `members` and `seeds` (two launches).
 * sgs_nbr_frontier: the sources edge_index[0][e] of the chosen ids that are not members yet become the next frontier: written ascending to
 *   frontier_out (nothing at or beyond cap), merged into the members; sizes_dev[0] = their number, sizes_dev[1] = the sum over them of
 *   min(next_fanout, in-degree) (next_fanout = -1: the in-degree; 0: not computed) -- what the next sgs_nbr_select will emit, so one 16-byte
 *   read-back per hop sizes both buffers.  Two launches: an atomic-OR pass over the chosen ids, a single-workgroup popcount scan over the words.
 * sgs_nbr_nodes: node_ids [n] int64 = the members ascending (a node's local id is its rank there), wpre [ceil(N / 32)] int32 = the members
 *   below each word; *mismatch_dev (may be NULL) is set to 1 if the members are not n.  One launch.
 * sgs_nbr_induced_count / _fill: every stored edge with both ends among the members, in ascending edge id: count per out-CSR row of the
 *   members and scan (rowptr [n + 1] int64, *total_dev = E_b; two launches), then fill edge_index_out [2, E_b] (local ids), prob_out = prob[id]
 *   and eid_out = id (either may be NULL) (one launch).  One wave per row, a row of more than sgs_nbr_select_hub_row() entries by the four
 *   waves of its workgroup together (the row squeeze of sgs_cluster_collate, csrc/batch_rows.h); membership and local ids from the bitmap
 *   and wpre.  rowptr holds the row counts between the two launches of the count; nothing is written outside [0, E_b) of an output.
 * sgs_nbr_directional: the chosen ids of all hops (segments_host [n_segments][2] = {device address of int32 ids, count}, by value; at most
 *   sgs_nbr_max_hops() segments, m ids in all), ascending, as edges: edge_index_out [2, m] (row stride m), prob_out, eid_out.  An id outside
 *   [0, E) or with an end outside the members is dropped; *total_dev = the number kept (the first *total_dev columns are written).  Uses the
 *   library radix sort, so the call is not capturable.  ws: sgs_nbr_directional_workspace_bytes(m), 8-byte aligned.
 * sgs_nbr_gather: one launch gathers, for the n members, x rows (row_bytes a multiple of 4), y (int64), masks [3, N] -> masks_out [3, n]
 *   ANDed with "is a seed", and seed_mask_out [n] (bytes).
 * Argument errors (SGS_EINVAL, message in sgs_last_error): N outside [1, 2^31); E, nnz, n_rows, m negative or >= 2^31; fanout 0 or below -1;
 *   n above N; a misaligned or null pointer; segments that do not add up to m.  SGS_EWORKSPACE: state or workspace too small. */
int64_t sgs_nbr_select_hub_row(void);
int sgs_nbr_max_hops(void);
size_t sgs_nbr_select_workspace_bytes(int64_t n_rows);
int sgs_nbr_select(const int32_t* in_ptr, const int32_t* in_eid, int64_t N, int64_t nnz, const int32_t* rows, int64_t n_rows, int64_t fanout,
                   uint32_t key, int32_t* chosen, int64_t cap, int64_t* total_dev, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_nbr_select_weighted(const int32_t* in_ptr, const int32_t* in_eid, const int32_t* in_wq, int64_t N, int64_t nnz, const int32_t* rows,
                            int64_t n_rows, int64_t fanout, uint32_t key, int32_t* chosen, int64_t cap, int64_t* total_dev, void* ws,
                            size_t ws_bytes, sgs_stream_t stream);
void sgs_nbr_log2_table(int32_t* out /* [257] */);
uint32_t sgs_nbr_weighted_key(uint32_t hash, uint32_t wq);
size_t sgs_nbr_state_bytes(int64_t N);
int sgs_nbr_begin(const int32_t* seeds, int64_t n_seeds, int64_t N, void* state, size_t state_bytes, sgs_stream_t stream);
int sgs_nbr_frontier(const int32_t* chosen, int64_t n_chosen, const int64_t* edge_index, int64_t E, int64_t N, const int32_t* in_ptr,
                     int64_t next_fanout, void* state, size_t state_bytes, int32_t* frontier_out, int64_t cap, int64_t* sizes_dev,
                     sgs_stream_t stream);
int sgs_nbr_nodes(const void* state, size_t state_bytes, int64_t N, int64_t n, int32_t* wpre, int64_t* node_ids, int32_t* mismatch_dev,
                  sgs_stream_t stream);
int sgs_nbr_induced_count(const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, int64_t N, int64_t E, const void* state,
                          size_t state_bytes, const int32_t* wpre, const int64_t* node_ids, int64_t n, int64_t* rowptr, int64_t* total_dev,
                          sgs_stream_t stream);
int sgs_nbr_induced_fill(const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, const float* prob, int64_t N, int64_t E,
                         const void* state, size_t state_bytes, const int32_t* wpre, const int64_t* node_ids, int64_t n, const int64_t* rowptr,
                         int64_t E_b, int64_t* edge_index_out, float* prob_out, int64_t* eid_out, sgs_stream_t stream);
size_t sgs_nbr_directional_workspace_bytes(int64_t m);
int sgs_nbr_directional(const int64_t* segments_host, int64_t n_segments, int64_t m, const int64_t* edge_index, int64_t E, int64_t N,
                        const float* prob, const void* state, size_t state_bytes, const int32_t* wpre, int64_t* edge_index_out, float* prob_out,
                        int64_t* eid_out, int64_t* total_dev, void* ws, size_t ws_bytes, sgs_stream_t stream);
int sgs_nbr_gather(const int64_t* node_ids, int64_t n, int64_t N, const void* x, int64_t row_bytes, void* x_out, const int64_t* y, int64_t* y_out,
                   const uint8_t* masks, const void* state, size_t state_bytes, uint8_t* masks_out, uint8_t* seed_mask_out, sgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SGS_HIP_H_ */
