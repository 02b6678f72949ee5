/* libribca_hip.so -- C ABI of the MI355X-native RIBCA hot path (gfx950 only).
 *
 * The reference (sun-huangqingbo/multiplexed-image-annotator) is pure Python and has no FFI: its compute boundary is a
 * set of Python methods.  Each entry point below replaces the body of one of them; the Python host in
 * multiplexed-image-annotator_amd/ binds these symbols with ctypes and keeps the reference's class/method surface
 * (INTEGRATION.md shows the stub a maintainer would add to the reference).  Paths cited are relative to
 * src/multiplexed_image_annotator/cell_type_annotation/ of the reference.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named *_host; sizes are element counts unless named *_bytes;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work and return;
 *   - the caller owns all memory; only ribca_vit_create allocates (the packed-weight handle);
 *   - return value 0 = ok, non-zero = error, text via ribca_last_error() (thread-local).  A request the library has no kernel for (a shape,
 *     a geometry, an attribute the runtime refuses) is such an error: no entry point ends the calling process, whatever it is handed
 *     (the reference's convention for a bad request is an exception the caller can catch: model.py:636, 770).
 *   - the kernel-level hooks tests/ and tools/ drive are NOT part of this ABI: include/ribca_hip_test.h, libribca_hip_test.so.
 */
#ifndef RIBCA_HIP_H
#define RIBCA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: the declarations between this push and the pop are its whole dynamic symbol table */
#pragma GCC visibility push(default)

typedef struct ribca_vit ribca_vit_t;
typedef struct ribca_mae ribca_mae_t;

int ribca_version(void);
const char* ribca_last_error(void);

/* ---- pre-processing ------------------------------------------------------------------------------------------ */

/* out2[0] = max(mask), out2[1] = min(mask).  Sizes the label table (preprocess.py:159-181 builds a dict instead). */
int ribca_mask_minmax(const int32_t* mask, int64_t n, int32_t* out2, void* stream);

/* Replaces ImageProcessor._cell_pos_dict (preprocess.py:159-211) for everything the hot path reads from it.
 * L = max label + 1.  tab_i32 = [5][L]: row min, row max, col min, col max, pixel count (count 0 = label absent);
 * tab_u64 = [2][L]: sum of rows, sum of cols.  Label 0 (background) is skipped; labels must be in [1, L). */
int ribca_label_table(const int32_t* mask, int32_t H, int32_t W, int32_t L, int32_t* tab_i32, uint64_t* tab_u64, void* stream);

/* Replaces ImageProcessor._move_image_range (preprocess.py:153-157): per-channel minimum of an fp32 (C, H*W) image. */
int ribca_channel_min(const float* image, int32_t C, int64_t hw, float* out_min, void* stream);

/* Replaces utils.crop_cell + utils.smooth (utils.py:226-270) for patch_size 40 (cell_size 30): for each of n cells writes
 * the soft-masked fp32 patch of EVERY image channel, (n, C, 40, 40), bit-identical to the reference arithmetic, and
 * optionally avg (n, C) fp64 = mean over labelled pixels of the window (reference avg_int, before the (x+1)/2 of
 * preprocess.py:145-149).  bbox = (n, 4) int32 rmin, rmax, cmin, cmax from the label table.  taps = 27 fp64 Gaussian
 * weights: sigma 1 -> taps[0..4], sigma 2 -> taps[5..13], sigma 3 -> taps[14..26], entry k = weight at distance k
 * (host computes them exactly as scipy.ndimage._gaussian_kernel1d does). */
int ribca_extract_patches(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const float* chan_min,
                          const int32_t* cell_id, const int32_t* bbox, const double* taps, int32_t n, float* patches, double* avg,
                          void* stream);

/* Same for cell_size != 30 (preprocess.py:78,106): window patch_size = int(40 * cell_size / 30), then
 * skimage.transform.resize(patch, (C, 40, 40), order=0, anti_aliasing=True, preserve_range=True): fp64 Gaussian pre-filter
 * (aa_taps[0..aa_radius], weight at distance k, sigma = (patch_size/40 - 1)/2; aa_radius = 0 when patch_size <= 40) in
 * 'mirror' mode, nearest-neighbour grid sampling at src_index[0..39] (host: floor(((o + 0.5) * patch_size/40 - 0.5) + 0.5) in
 * fp64, as scipy.ndimage.zoom(order=0, grid_mode=True)), one rounding to fp32.  avg is taken over the patch_size window
 * before the resize, as crop_cell does.  4 <= patch_size <= 90. */
int ribca_extract_patches_scaled(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const float* chan_min,
                                 const int32_t* cell_id, const int32_t* bbox, const double* taps, int32_t n, int32_t patch_size,
                                 const double* aa_taps, int32_t aa_radius, const int32_t* src_index, float* patches, double* avg,
                                 void* stream);

/* ---- whole-image normalisation primitives (ImageProcessor._normalize, preprocess.py:214-239) ---------------------
 * The host drives them per image (ops.normalize_image in the Python package shows the sequence): the percentile needs
 * a data-dependent host decision, everything touching pixels runs here.  Results are bit-identical to the reference. */
int ribca_u16_to_f32(const uint16_t* in, float* out, int64_t n, void* stream);
/* One axis of scipy.ndimage.gaussian_filter on `planes` fp32 (H, W) images: fp64 accumulation in scipy's order, fp32 result.
 * taps[k] = weight at distance k (k = 0..R); mode 0 = 'reflect', 1 = 'nearest'; axis 0 = rows, 1 = columns; in != out. */
int ribca_gauss1d(const float* in, float* out, int32_t planes, int32_t H, int32_t W, int32_t axis, const double* taps, int32_t R,
                  int32_t mode, void* stream);
/* x = max(x - min(bg, cap), 0) (preprocess.py:219-222) */
int ribca_bg_subtract(float* x, const float* bg, int64_t n, float cap, void* stream);
/* out[p] = max over plane p of non-negative fp32 data */
int ribca_plane_max(const float* x, int32_t planes, int64_t hw, float* out, void* stream);
/* One radix-select pass over non-negative fp32 keys: hist[p][b] = #{k in plane p : (k & mask_hi) == prefix[p],
 * (k >> shift) & (2^bits - 1) == b}; hist is (planes, 2048) uint32.  Three passes (11 + 11 + 10 bits) locate any order
 * statistic exactly; np.percentile's interpolation between two of them is done by the host. */
int ribca_radix_hist(const float* x, int32_t planes, int64_t hw, const uint32_t* prefix, uint32_t mask_hi, int32_t shift, int32_t bits,
                     uint32_t* hist, void* stream);
/* per plane: mode 0 -> fill -1; else x = 2 * (min(x, clip) / denom) - 1 (preprocess.py:229-238) */
int ribca_norm_finalize(float* x, int32_t planes, int64_t hw, const int32_t* mode, const float* clip, const float* denom, void* stream);

/* ---- ViT classifier (timm VisionTransformer subclass, model.py:31-88) -------------------------------------- */

/* Number of fp32 values in the flat parameter blob ribca_vit_create expects, in this order:
 *   cls_token[D], pos_embed[101*D], patch_embed.proj.weight[D*C*16], patch_embed.proj.bias[D],
 *   per block: norm1.weight[D], norm1.bias[D], attn.qkv.weight[3D*D], attn.qkv.bias[3D], attn.proj.weight[D*D],
 *              attn.proj.bias[D], norm2.weight[D], norm2.bias[D], mlp.fc1.weight[4D*D], mlp.fc1.bias[4D],
 *              mlp.fc2.weight[D*4D], mlp.fc2.bias[D],
 *   norm.weight[D], norm.bias[D], head.weight[K*D], head.bias[K]
 * (the state-dict key order of the checkpoints Annotator.load_models reads, model.py:188-239). */
/* 1 if classifiers of width D run mlp.fc1 -> mlp.fc2 as the MX pair (csrc/gemm_mx.hip: fp16 hi * hi + two block-scaled corrections, 1.75
 * matrix units per product and 3 bytes per element of h instead of 3 passes / 4 bytes): 4 D % 128 == 0, D % 48 == 0 and RIBCA_MX != 0 */
int32_t ribca_mx_enabled(int32_t D);
/* 1 if, beyond that, the residual rows of a classifier of width D are ALSO kept in the MX3 format and attn.qkv (where it is a GEMM of its own)
 * and mlp.fc1 run on the MX kernel too: ribca_mx_enabled(D), D % 192 == 0 and RIBCA_MXZ != 0 */
int32_t ribca_mxz_enabled(int32_t D);
int64_t ribca_vit_blob_len(int32_t D, int32_t C, int32_t K, int32_t depth);

/* Replaces Annotator.load_models for one model: repacks the fp32 parameters (device blob) into the MFMA layouts.
 * D % 48 == 0 (12 heads, head dim % 4 == 0), D <= 768, K <= 16. */
int ribca_vit_create(const float* blob, int64_t blob_len, int32_t D, int32_t C, int32_t K, int32_t depth, void* stream,
                     ribca_vit_t** out);
void ribca_vit_destroy(ribca_vit_t* m);
/* The fast level of ribca_vit_forward for this handle.  2 (what create sets): every MX product the width allows, among them the QKV phase of
 * the fused per-cell kernel (csrc/cell_attention_mx.hip; D = 384, RIBCA_CELL_ATTN_MX != 0); 1: that kernel at three fp16 passes
 * (csrc/cell_attention.hip), every other product as at level 2.  A load-time probe that refuses level 2 for a model's weights can so keep the
 * model's fc1 / fc2 MX products.  Returns the level in effect (1 where the handle has no per-cell MX kernel to switch off), -1 on a bad
 * argument.  Arena and workspace sizes do not depend on the level; ribca_vit_forward_precise is untouched by it.  Not thread-safe against a
 * forward of the same handle. */
int32_t ribca_vit_set_fast_level(ribca_vit_t* m, int32_t level);

/* Scratch bytes ribca_vit_forward needs to process `chunk_cells` cells at a time. */
int64_t ribca_vit_workspace_bytes(const ribca_vit_t* m, int32_t chunk_cells);

/* Replaces the body of Annotator._predict_cell_types' inner loop (model.py:397-406): probs = softmax(model(x), dim=1).
 * patches: (n_cells, c_img, 40, 40) fp32 full-channel patches from ribca_extract_patches (or the imputer);
 * src_chan: (C) int32, image channel feeding each model channel, -1 = blank plane of -1.0 (preprocess.py:110-120);
 * probs: (n_cells, K) fp32.  Cells are processed in chunks of chunk_cells through `workspace`. */
int ribca_vit_forward(const ribca_vit_t* m, const float* patches, int32_t c_img, const int32_t* src_chan, int32_t n_cells,
                      float* probs, void* workspace, int64_t workspace_bytes, int32_t chunk_cells, void* stream);
/* The same forward with every product as three fp16 passes (the 22-bit operands of round 3), whatever ribca_mx_enabled says: what
 * Annotator.predict re-evaluates the few cells with whose fast result lies within the MX arithmetic's error of a decision boundary
 * (top-2 margin, confidence thresholds), so that labels are those of the full-precision path.  Same arguments, same workspace. */
int ribca_vit_forward_precise(const ribca_vit_t* m, const float* patches, int32_t c_img, const int32_t* src_chan, int32_t n_cells,
                      float* probs, void* workspace, int64_t workspace_bytes, int32_t chunk_cells, void* stream);

/* Algorithmic FLOPs per cell of this model (BASELINE.md section 3 formula). */
double ribca_vit_flops_per_cell(const ribca_vit_t* m);

/* ---- marker imputer (MarkerImputer / MaskedAutoencoderViT, markerImputer.py:69-329) --------------------------------
 * Tokens are the panel's L channels (each 40x40 plane = 1600 pixels); encoder 768 wide / 12 heads over the present
 * channels + CLS, decoder 512 / 8 heads over all L + CLS, linear prediction of the missing planes.
 * Blob order (state-dict keys of the *_impute.pth checkpoints): cls_token[768], pos_embed[(L+1)*768],
 * patch_embed.proj.weight[768*1600], patch_embed.proj.bias[768], blocks.* (same 12 tensors per block as the classifier),
 * norm.weight, norm.bias, decoder_embed.weight[512*768], decoder_embed.bias[512], mask_token[512],
 * decoder_pos_embed[(L+1)*512], decoder_blocks.*, decoder_norm.weight, decoder_norm.bias,
 * decoder_pred.weight[1600*512], decoder_pred.bias[1600]. */
int64_t ribca_mae_blob_len(int32_t L, int32_t enc_depth, int32_t dec_depth);
int ribca_mae_create(const float* blob, int64_t blob_len, int32_t L, int32_t enc_depth, int32_t dec_depth, void* stream,
                     ribca_mae_t** out);
/* The same with the block path as an argument instead of the environment.  fold = 1: folded blocks (LayerNorm folded into qkv / fc1,
 * packed-split residual stream, MX products where the width allows); fold = 0: fp32 residual stream, LayerNorm kernels, every product
 * as three fp16 passes (the yardstick of the load-time probe and the fallback for weights it refuses).  Any other value is refused.
 * ribca_mae_create = this with fold = 0 where RIBCA_MAE_FOLD=0 is set in the environment at that call, else 1. */
int ribca_mae_create_path(const float* blob, int64_t blob_len, int32_t L, int32_t enc_depth, int32_t dec_depth, int32_t fold, void* stream,
                          ribca_mae_t** out);
void ribca_mae_destroy(ribca_mae_t* m);
int64_t ribca_mae_workspace_bytes(const ribca_mae_t* m, int32_t chunk_cells, int32_t n_present);
/* Replaces MarkerImputer.impute (markerImputer.py:294-329): patches (n_cells, L, 40, 40) fp32 in place -- every channel
 * position NOT listed in present_host (HOST array, strictly increasing, n_present entries) is overwritten by the
 * prediction; listed channels are left bit-for-bit untouched.  Synchronises the stream once (index tables upload). */
int ribca_mae_impute(const ribca_mae_t* m, float* patches, const int32_t* present_host, int32_t n_present, int32_t n_cells,
                     void* workspace, int64_t workspace_bytes, int32_t chunk_cells, void* stream);

/* ---- label painting (Annotator.colorize, model.py:806-858, without tissue regions) ---------------------------------
 * mask (n_pixels) int32; label_to_cell (L) int32: row of the label in the per-cell arrays or -1; per-cell colours
 * cell_type_rgb / cell_conf_rgb (n_cells, 3) uint8 and cell_type_idx (n_cells) uint8 (= cell-type index + 1).
 * Outputs: (n_pixels, 3), (n_pixels, 3), (n_pixels) uint8; background and unknown labels are 0. */
int ribca_colorize(const int32_t* mask, int64_t n_pixels, const int32_t* label_to_cell, int32_t L, const uint8_t* cell_type_rgb,
                   const uint8_t* cell_conf_rgb, const uint8_t* cell_type_idx, uint8_t* out_type_rgb, uint8_t* out_conf_rgb,
                   uint8_t* out_type_idx, void* stream);

/* ---- neighbourhood analysis (spatial_methods.neighborhood_analysis, spatial_methods.py:13-130) ------------------------
 * x, y (n_cells) fp64 cell centroids (mean column, mean row), cell_type (n_cells) int32 in [0, n_types).  For every cell the
 * n_neighbors nearest cells in fp64 (itself first; ties towards the lower index -- the reference's ball tree leaves ties
 * unspecified) and matrix[type(cell)][type(neighbour)] += 1 for the other n_neighbors - 1.  matrix (n_types, n_types) uint64 is
 * ACCUMULATED into (zero it first; call once per image for the integrated mode).  n_neighbors <= 32, n_types <= 254 (the most the uint8
 * index image of ribca_colorize holds; up to 32 types the counts go through an LDS histogram, above that straight to matrix with integer
 * atomics -- either way order-independent, so the result is deterministic). */
int ribca_knn_cooccurrence(const double* x, const double* y, const int32_t* cell_type, int32_t n_cells, int32_t n_neighbors, int32_t n_types,
                           uint64_t* matrix, void* stream);

/* The neighbour list of the same search: idx (n, k - 1) int32, idx[i][p - 1] = the cell of rank p = 1 .. k - 1 among the k nearest of cell i
 * (rank 0, the cell itself -- or the lower index among exact duplicates -- is dropped), by (fp64 dx*dx + dy*dy, index).  Counting
 * matrix[type[i]][type[idx[i][q]]] over the list gives ribca_knn_cooccurrence's matrix.  2 <= k <= min(n, 32). */
int ribca_knn_neighbours(const double* x, const double* y, int32_t n, int32_t k, int32_t* idx, void* stream);

/* ---- neighbourhood enrichment: the permutation null of the co-occurrence counts (csrc/enrichment.hip) ----------------
 * The graph stays, the labels move: for the permutation with the global index p = p0 + j, j = 0 .. P - 1, cell i carries
 * label_p(i) = cell_type[sigma_p(i)] and counts[j][label_p(i)][label_p(idx[i][q])] += 1 for q = 0 .. m - 1.  idx (n, m) int32 (entries outside
 * [0, n) are skipped), cell_type (n) int32 (values outside [0, T) are skipped, as either end of a pair), counts (P, T, T) uint64, ACCUMULATED
 * into (zero it first; call once per image of a group).  Integer atomics only: the result does not depend on the launch geometry.
 * sigma_p is a keyed bijection of [0, n), a six-round balanced Feistel network with cycle walking, all in uint64:
 *     s(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *     h = max(1, (bit_length(n - 1) + 1) / 2), mask = 2^h - 1;   K = s(s(s(seed) ^ image) ^ p)
 *     one pass on v < 4^h: L = v >> h, R = v & mask; for r = 0 .. 5: f = s(K ^ ((r << 32) | R)) >> (64 - h), (L, R) = (R, L ^ f); v = (L << h) | R
 *     sigma_p(i): v = i; repeat the pass until v < n (at most 4^h - n + 1 passes: the walk stays on the cycle of i).
 * 1 <= n <= 2^30, 1 <= m <= 31, 1 <= T <= 64, image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31.  ws: ribca_nhood_perm_counts_ws_bytes(n, P) bytes (the
 * shuffled labels of a batch of permutations, one byte per cell; 0 for arguments the entry point refuses).  Does not synchronise. */
int64_t ribca_nhood_perm_counts_ws_bytes(int32_t n, int32_t P);
int ribca_nhood_perm_counts(const int32_t* idx, const int32_t* cell_type, int32_t n, int32_t m, int32_t T, uint64_t seed, int32_t image, int64_t p0,
                            int32_t P, uint64_t* counts, void* ws, int64_t ws_bytes, void* stream);

/* ---- spatial autocorrelation of the markers: the numerators of Moran's I and Geary's C, observed and under a permutation null
 * (csrc/autocorr.hip) ---------------------------------------------------------------------------------------------------
 * z (n, C) fp64 row-major: the caller's CENTRED values (nothing is centred here); idx (n, m) int32: the neighbour list (entries outside [0, n)
 * are skipped, by an unsigned compare before they index anything).  For the permutation with the global index p = p0 + j, j = 0 .. P - 1, cell i
 * carries the whole row zp[i] = z[sigma_p(i)]: one sigma_p serves all channels, and it is the bijection stated under ribca_nhood_perm_counts
 * with the same key K = s(s(s(seed) ^ image) ^ p).  ribca_autocorr_observed is the same with sigma the identity (zp = z).  Per channel c, every
 * operation rounded on its own (no fma), no floating-point atomic anywhere:
 *     s_i = (((+0.0 + zp[j_0][c]) + zp[j_1][c]) + ...)   over the valid entries j_q = idx[i][q], q ascending
 *     g_i = (((+0.0 + d_0 * d_0) + d_1 * d_1) + ...),    d_q = zp[i][c] - zp[j_q][c], over the same entries
 *     a_i = zp[i][c] * s_i
 *     out[j][0][c] = TREE(a),  out[j][1][c] = TREE(g)     (the numerators of Moran's I and of Geary's C)
 * TREE(v), R = 256: chunk k = the cells [k R, (k + 1) R), padded with +0.0 past n; eight rounds of adjacent pairs, v = v[0::2] + v[1::2], leave
 * part[k]; the total is (((+0.0 + part[0]) + part[1]) + ...) over ALL chunks in ascending k.  In numpy:
 *     v = np.concatenate([v, np.zeros(chunks * 256 - n)]).reshape(chunks, 256);  for r in range(8): v = v[:, 0::2] + v[:, 1::2]
 *     total = 0.0;  for k in range(chunks): total = total + v[k, 0]
 * out -- (2, C) fp64 for ribca_autocorr_observed, (P, 2, C) for ribca_autocorr_perm -- is OVERWRITTEN, not accumulated: the caller fixes the
 * order in which the images of a group are added, as ribca_group_sums leaves it to the caller.  It is a pure function of (z, idx, seed, image, p):
 * it does not depend on p0, P, the internal batch of permutations, the launch geometry, the workspace contents, the device or the stream.
 * 1 <= n <= 2^30, 1 <= C <= 64, 1 <= m <= 31, image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31.  ws: ribca_autocorr_observed_ws_bytes(n, C) bytes (the
 * chunk partials) and ribca_autocorr_perm_ws_bytes(n, C, P) bytes (the permuted rows of a batch of B = min(P, 32, max(1, 64 MiB / (8 n L)))
 * permutations, kept in rows of L doubles -- L = the power of two >= C up to 16, the multiple of 16 >= C above -- and their chunk partials); both 0
 * for arguments the entry point refuses.  Neither synchronises. */
int64_t ribca_autocorr_observed_ws_bytes(int32_t n, int32_t C);
int ribca_autocorr_observed(const double* z, const int32_t* idx, int32_t n, int32_t C, int32_t m, double* out, void* ws, int64_t ws_bytes, void* stream);
int64_t ribca_autocorr_perm_ws_bytes(int32_t n, int32_t C, int32_t P);
int ribca_autocorr_perm(const double* z, const int32_t* idx, int32_t n, int32_t C, int32_t m, uint64_t seed, int32_t image, int64_t p0, int32_t P,
                        double* out, void* ws, int64_t ws_bytes, void* stream);

/* ---- local indicators of spatial association: per cell and channel the neighbour sum and its conditional-permutation counts
 * (csrc/local_autocorr.hip) ---------------------------------------------------------------------------------------------
 * z (n, C) fp64 row-major, the caller's CENTRED values, and idx (n, m) int32, the neighbour list, as for ribca_autocorr_observed: entries outside
 * [0, n) are skipped, by an unsigned compare before they index anything.  Every operation rounded on its own (no fma), no floating-point atomic.
 *     lag[i][c] = (((+0.0 + z[j_0][c]) + z[j_1][c]) + ...)   over the valid entries j_q = idx[i][q], q ascending        (ribca_local_lag)
 * Conditional permutation p = p0 + b, b = 0 .. P - 1: cell i keeps its own row and the other n - 1 rows are permuted around it by sigma_p, the
 * bijection stated under ribca_nhood_perm_counts with the same key K = s(s(s(seed) ^ image) ^ p), followed by the swap that fixes i.  For a valid
 * entry j of the list of i the source row is, by the first rule that matches,
 *     i if j == i;   sigma_p(i) if sigma_p(j) == i;   sigma_p(j) otherwise
 * (tau o sigma_p with tau the transposition (i, sigma_p(i)): a bijection with the fixed point i, so distinct entries j != i draw distinct other
 * cells), and s_p[i][c] is the same ordered sum over z[source][c].  Then
 *     ge[i][c] = the number of p in [p0, p0 + P) with s_p[i][c] >= lag[i][c],     le[i][c] = the same with <=
 * ge, le (n, C) uint32 are OVERWRITTEN; lag (n, C) fp64 is an INPUT of ribca_local_perm_counts (what ribca_local_lag wrote).  The counts are a
 * pure function of (z, idx, lag, seed, image, p0, P): counts over [p0, p0 + P) equal counts over [p0, p0 + Q) plus counts over [p0 + Q, p0 + P),
 * entry by entry, and nothing depends on the internal batch, the launch geometry, the workspace contents, the device or the stream.
 * 1 <= n <= 2^30, 1 <= C <= 64, 1 <= m <= 31, image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31.  ws: ribca_local_perm_counts_ws_bytes(n, C, P) bytes,
 * two pieces, each rounded up to 256 bytes: the permuted rows of a batch of B = min(P, 32, max(1, 64 MiB / (8 n L))) permutations, 8 B n L bytes
 * (L as for ribca_autocorr_perm: the power of two >= C up to 16, the multiple of 16 >= C above), and the inverse of sigma for each of them, 4 B n
 * bytes; 0 for arguments the entry point refuses.  Neither entry point synchronises. */
int ribca_local_lag(const double* z, const int32_t* idx, int32_t n, int32_t C, int32_t m, double* lag, void* stream);
int64_t ribca_local_perm_counts_ws_bytes(int32_t n, int32_t C, int32_t P);
int ribca_local_perm_counts(const double* z, const int32_t* idx, const double* lag, int32_t n, int32_t C, int32_t m, uint64_t seed, int32_t image,
                            int64_t p0, int32_t P, uint32_t* ge, uint32_t* le, void* ws, int64_t ws_bytes, void* stream);

/* ---- co-occurrence by distance: cell-type pair counts per radius band (csrc/cooccurrence.hip) ---------------------------
 * x, y (n) fp64, cell_type (n) int32 on the device; r2_host: a HOST array of the B squared radii, finite, non-negative and strictly increasing,
 * 1 <= B <= 32 (passed to the kernel by value, as ribca_mae_impute takes present_host).  For every ORDERED pair i != j whose labels both lie in
 * [0, T): counts[b][cell_type[i]][cell_type[j]] += 1 for the one band b with r2[b - 1] < d2 <= r2[b] (band 0: d2 <= r2[0]; a pair beyond
 * r2[B - 1] is not counted; a label outside [0, T) is skipped on either side).  d2 in fp64 exactly as the k-NN search forms it: dx = x_i - x_j,
 * d = dx * dx, d += dy * dy, every operation rounded on its own -- a numpy loop reproduces each comparison, ties at a band edge included (the <=
 * is inclusive).  counts (B, T, T) uint64 is ACCUMULATED into (zero it first; call once per image of a group).  Integer atomics only: the result
 * does not depend on the launch geometry.  While B T T 32-bit counters fit 64 KiB they are kept in LDS per workgroup, above that (up to T = 254)
 * every count goes straight to counts.  1 <= n <= 2^21 (the work is quadratic: 4.4e12 pairs at the cap), 1 <= T <= 254.  No workspace:
 * ribca_radial_pair_counts_ws_bytes returns 0 and ws may be NULL.  Does not synchronise. */
int64_t ribca_radial_pair_counts_ws_bytes(int32_t n, int32_t T, int32_t B);
int ribca_radial_pair_counts(const double* x, const double* y, const int32_t* cell_type, int32_t n, int32_t T, const double* r2_host, int32_t B,
                             uint64_t* counts, void* ws, int64_t ws_bytes, void* stream);

/* ---- nearest cell of every type: per-cell distances and the cross-type G function under a label null (csrc/nearest.hip) --
 * x, y (n) fp64 (finite), cell_type (n) int32 on the device.  d2(i, j) in fp64 exactly as ribca_radial_pair_counts forms it: dx = x_i - x_j,
 * dy = y_i - y_j, d2 = dx * dx + dy * dy with the two products and the sum each rounded on its own (no fma) -- a numpy loop reproduces every
 * comparison.
 * ribca_nearest_by_type: for every cell i and every type b in [0, T)
 *     near2[i][b] = min of d2(i, j) over j != i with cell_type[j] == b,  +inf if there is no such cell
 *     arg[i][b]   = the LOWEST such j that attains the minimum,           -1 if there is none
 * near2 (n, T) fp64 and arg (n, T) int32 are OVERWRITTEN.  A label outside [0, T) is never a target, but its cell still gets a row.  Exact
 * duplicates are distinct cells: d2 == 0 is a valid minimum.  1 <= n <= 2^21 (the work is quadratic, the cap of ribca_radial_pair_counts),
 * 1 <= T <= 254.
 * ribca_nearest_perm_counts: r2_host is a HOST array of the B squared radii, finite, non-negative and strictly increasing, 1 <= B <= 32, as for
 * ribca_radial_pair_counts.  The positions stay, the labels move: for the permutation with the global index p = p0 + j, j = 0 .. P - 1, cell i
 * carries label_p(i) = cell_type[sigma_p(i)], sigma_p the bijection stated under ribca_nhood_perm_counts with the same key
 * K = s(s(s(seed) ^ image) ^ p).  For every cell i with a = label_p(i) in [0, T) and every b in [0, T):
 *     m = min of d2(i, k) over k != i with label_p(k) == b;   if m <= r2[B - 1]: counts[j][band][a][b] += 1
 * for the one band with r2[band - 1] < m <= r2[band] (band 0: m <= r2[0]); otherwise, or if no other cell carries b, nothing is counted.  A label
 * outside [0, T) is skipped as a query and as a target.  counts (P, B, T, T) uint64 is ACCUMULATED into (zero it first; call once per image of a
 * group); the bands are not cumulative.  Under the identity labelling the same rule applied to near2 gives the observed counts.  The result is a
 * pure function of (x, y, cell_type, r2, seed, image, p): it does not depend on p0, P, the internal batch of permutations, the launch geometry,
 * the workspace contents or the stream.  Integer atomics only, no floating-point atomic anywhere.  1 <= n <= 2^21, 1 <= T <= 64, image >= 0,
 * p0 >= 0, 1 <= P, p0 + P <= 2^31.
 * ws: ribca_nearest_by_type_ws_bytes(n, T) and ribca_nearest_perm_counts_ws_bytes(n, T, P) bytes, six pieces, each rounded up to 256 bytes: the
 * counting sort of the cells by (type, index) -- 1024 bytes per chunk of 1024 cells, 4 (T + 2) bytes of segment offsets, three int32 arrays of n
 * (the slot of a cell, the cell of a slot, the segment of a slot) -- and the coordinates in slot order, 16 n bytes, for the permutation counts one
 * copy for each of a batch of min(P, 32, max(1, 64 MiB / (16 n))) permutations; both 0 for arguments the entry point refuses.  Neither entry
 * point synchronises. */
int64_t ribca_nearest_by_type_ws_bytes(int32_t n, int32_t T);
int ribca_nearest_by_type(const double* x, const double* y, const int32_t* cell_type, int32_t n, int32_t T, double* near2, int32_t* arg, void* ws,
                          int64_t ws_bytes, void* stream);
int64_t ribca_nearest_perm_counts_ws_bytes(int32_t n, int32_t T, int32_t P);
int ribca_nearest_perm_counts(const double* x, const double* y, const int32_t* cell_type, int32_t n, int32_t T, const double* r2_host, int32_t B,
                              uint64_t seed, int32_t image, int64_t p0, int32_t P, uint64_t* counts, void* ws, int64_t ws_bytes, void* stream);

/* ---- cell contact graph of the segmentation mask and the label null over an edge list (csrc/contact.hip) ---------------
 * mask (H, W) int32 row-major and label_to_cell (L) int32 on the device.  The pixel p belongs to the cell c = label_to_cell[mask[p]] when
 * 0 <= mask[p] < L and 0 <= c < n, and to no cell otherwise (negative labels, labels >= L, labels mapped outside [0, n); the background label 0
 * is excluded by mapping it to -1, as ops.contact_graph does).  A label in two blobs is one cell.  For the integer reach d, 1 <= d <= 8,
 *     w(i, j) = #{ (p, q) : cell(p) = i, cell(q) = j, i != j, (p_r - q_r)^2 + (p_c - q_c)^2 <= d^2 }
 * the ordered pixel pairs within the Euclidean disk, all in integers (4, 12, 28, 48, 80, 112, 148, 196 offsets for d = 1 .. 8; at d = 1 the shared
 * border in pixel edges); nothing outside the image is read.  w is symmetric, and i and j are IN CONTACT iff w(i, j) > 0.
 * ribca_contact_table: nbr (n, S) int32, pairs (n, S) uint64, degree (n) int32 and over (2) int32 are all OVERWRITTEN (the library initialises
 * them and its workspace itself).  over[0] == 0: degree[i] = the number of cells in contact with i; nbr[i][0 .. degree[i]) holds them in ASCENDING
 * index order with w(i, .) beside them in pairs; the rest of either row is -1 / 0; over[1] = -1.  over[0] > 0: that many cells have more than S
 * neighbours, over[1] is the lowest such cell index, the other outputs are unspecified -- call again with a larger S.  The result is a pure
 * function of (mask, label_to_cell, d): the same for every S that fits, every launch geometry and every run (integer sums; the rows are sorted).
 * 1 <= H, W, H W < 2^31, 1 <= L, 1 <= n <= 2^21, S a power of two in 8 .. 1024.  ws: ribca_contact_table_ws_bytes(H, W, n, S) bytes, three
 * pieces, each rounded up to 256 bytes: the open-addressing table the kernels insert into, 4 n S bytes of keys and 8 n S bytes of sums, and 4 n
 * bytes of overflow flags; 0 for arguments the entry point refuses.  No loop of any kernel waits for another thread: every probe sequence ends
 * after at most S slots.
 * ribca_edge_perm_counts: the general graph form of the null of ribca_nhood_perm_counts.  src, dst (E) int32: directed edges.  For the permutation
 * with the global index p = p0 + j, j = 0 .. P - 1, cell i carries label_p(i) = cell_type[sigma_p(i)], sigma_p the bijection stated under
 * ribca_nhood_perm_counts with the same key K = s(s(s(seed) ^ image) ^ p), and counts[j][label_p(src[e])][label_p(dst[e])] += 1 for every edge e;
 * an edge with an end outside [0, n) or a label outside [0, T) is skipped.  counts (P, T, T) uint64 is ACCUMULATED into (zero it first; call once
 * per image of a group).  Integer atomics only; a pure function of (src, dst, cell_type, seed, image, p): a split of the permutation range is
 * invisible.  1 <= E < 2^31, 1 <= n <= 2^30, 1 <= T <= 64, image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31.  ws: ribca_edge_perm_counts_ws_bytes(n, P)
 * bytes, the shuffled labels of a batch of min(P, 128, max(1, 64 MiB / n)) permutations, one byte per cell; 0 for arguments the entry point
 * refuses.  Neither entry point synchronises. */
int64_t ribca_contact_table_ws_bytes(int32_t H, int32_t W, int32_t n, int32_t S);
int ribca_contact_table(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, int32_t d, int32_t S,
                        int32_t* nbr, uint64_t* pairs, int32_t* degree, int32_t* over, void* ws, int64_t ws_bytes, void* stream);
int64_t ribca_edge_perm_counts_ws_bytes(int32_t n, int32_t P);
int ribca_edge_perm_counts(const int32_t* src, const int32_t* dst, int64_t E, const int32_t* cell_type, int32_t n, int32_t T, uint64_t seed,
                           int32_t image, int64_t p0, int32_t P, uint64_t* counts, void* ws, int64_t ws_bytes, void* stream);

/* ---- per-cell morphology sums of the segmentation mask (csrc/morphology.hip) -----------------------------------------
 * mask (H, W) int32 row-major and label_to_cell (L) int32 on the device; pixel ownership is the rule of ribca_contact_table: the pixel p belongs to
 * the cell c = label_to_cell[mask[p]] when 0 <= mask[p] < L and 0 <= c < n, and to no cell otherwise; a label in several blobs is one cell.  With
 * S = the set of the pixels (r, c) of cell i, sums (n, 16) uint64 is OVERWRITTEN with
 *     0        the area |S|
 *     1, 2     sum r, sum c                    3, 4, 5   sum r^2, sum c^2, sum r c
 *     6, 7, 8  the 4-neighbour pixel edges that leave S -- one (pixel of S, neighbour) pair each -- into another cell / into no cell inside the
 *              image / out of the image; column 6 is the sum over j of w(i, j) of ribca_contact_table at d = 1
 *     9 .. 11  the perimeter classes p_a, p_b, p_c of scikit-image's perimeter(neighbourhood=4): a pixel of S is a BORDER pixel of i when one of
 *              its four neighbours is not in S (outside the image is not in S); for a border pixel, a = the number of its 4-neighbours that are
 *              border pixels of i, b = the same over its four diagonal neighbours, v = 1 + 2 a + 10 b; p_a counts v in {5, 7, 15, 17, 25, 27},
 *              p_b counts v in {21, 33}, p_c counts v in {13, 23}, every other v counts nowhere (perimeter = p_a + p_b sqrt 2 + p_c (1 + sqrt 2) / 2)
 *     12 .. 14 the bit-quad counts q1, q3, qd: over each of the (H + 1)(W + 1) 2 x 2 windows of the mask extended by one ring of "no cell", every
 *              window once, a cell that holds k of the window's four pixels counts q1 at k = 1, q3 at k = 3 and qd at k = 2 with the two on a
 *              diagonal; (q1 - q3 - 2 qd) / 4 is the Euler number at 8-connectivity: components (8-connected) minus holes (4-connected)
 *     15       the pixels of S with r0 <= r < r1 and c0 <= c < c1 of the cell's row (r0, r1, c0, c1) of rect (n, 4) int32 (any values; an empty
 *              rectangle counts nothing); 0 when rect is NULL
 * and bbox (n, 4) int32 is OVERWRITTEN with rmin, rmax, cmin, cmax (inclusive), (INT32_MAX, -1, INT32_MAX, -1) for a cell without a pixel.
 * Integer atomics only: a pure function of (mask, label_to_cell, rect), the same for every launch geometry and every run.  1 <= H, W <= 65535 (so
 * that sum r^2 stays below 2^63), H W < 2^31, 1 <= L, 1 <= n <= 2^21.  workspace: ribca_mask_morphology_ws_bytes(H, W, n) bytes; 0 for arguments the
 * entry point refuses.  The piece is RESERVED: 256 bytes today, and the present kernels accumulate in the outputs and neither read nor write
 * it; a NULL or short workspace is refused all the same, as for every entry point that takes one, so that a later form can use it.  No loop of the kernels waits for another thread.  The entry
 * point does not synchronise. */
int64_t ribca_mask_morphology_ws_bytes(int32_t H, int32_t W, int32_t n);
int ribca_mask_morphology(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, const int32_t* rect,
                          uint64_t* sums, int32_t* bbox, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- per-cell marker intensities over the cell's own pixels (csrc/intensities.hip) -------------------------------------
 * image (C, H, W) fp32, mask (H, W) int32, ids (n) int32 and bbox (n, 4) int32 on the device; q_num (Q) int32 is a HOST array, read before
 * the launch.  bbox holds rmin, rmax, cmin, cmax, all inclusive, in the form ribca_label_table writes; it is clipped to the image.  The
 * pixel set S of cell i is the pixels of its clipped box with mask == ids[i], in row-major order; ids[i] <= 0 or an empty box give an empty S
 * (a box that leaves out pixels of the label leaves them out of S).  With a = |S| and v_0 .. v_{a-1} a channel's values over S widened to fp64,
 * all three outputs are OVERWRITTEN:
 *     area  (n) int32          a
 *     sums  (n, C, 2) fp64     sum, ssd.  Partial p_j, j = 0 .. 255, starts at 0.0 and adds v_j, v_{j+256}, v_{j+512}, ... in that order; then for
 *                              s = 128, 64, ..., 1: p_j += p_{j+s} for j < s; sum = p_0 and m = sum / a.  ssd is the same tree over
 *                              (v_j - m) * (v_j - m); every operation is rounded on its own (no fused multiply-add)
 *     order (n, C, Q, 2) fp32  the values sorted by the total-order key of the fp32 bit pattern (all bits of a negative flipped, the sign bit of
 *                              the rest set: -0.0 < +0.0, ties are bit-identical); for quantile k with h = (a - 1) q_num[k] in 64-bit integers,
 *                              lo = h / q_den, hi = lo + (h % q_den != 0): order[i, c, k] = (x_(lo), x_(hi)), bit patterns preserved
 * a = 0 gives sum = ssd = 0 and the quiet NaN 0x7FC00000 in order.  For finite inputs the outputs are a pure function of the arguments, the same
 * for every launch geometry and every run (no floating-point atomics; the selection counts in integers); for non-finite values only order is
 * specified.  1 <= C <= 64, 1 <= Q <= 8, 1 <= q_den, 0 <= q_num[k] <= q_den, 1 <= H, W <= 65535, H W < 2^31, 1 <= n <= 2^21; n == 0 returns 0 and
 * touches nothing.  No workspace.  No loop of the kernel waits for another thread.  The entry point does not synchronise. */
int ribca_cell_intensities(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const int32_t* ids, const int32_t* bbox,
                           int32_t n, const int32_t* q_num, int32_t Q, int32_t q_den, int32_t* area, double* sums, float* order, void* stream);

/* ---- growing the labels of a mask by D pixels (csrc/expand.hip) ----------------------------------------------------------
 * mask (H, W) int32 row-major on the device, e.g. a nuclear segmentation; out (H, W) int32 and, unless NULL, dist2 (H, W) int32 are OVERWRITTEN.
 * A pixel p is LABELLED when mask[p] > 0: out[p] = mask[p], dist2[p] = 0.  A pixel q with mask[q] <= 0 is GROWN when some labelled pixel lies
 * within squared Euclidean distance D D of it: with m = the smallest squared distance from q to a labelled pixel, out[q] = the SMALLEST label value
 * among the labelled pixels at squared distance exactly m, and dist2[q] = m.  A pixel that is neither gets out[q] = mask[q] -- zeros and
 * negatives pass through -- and dist2[q] = -1.  Nothing outside the image is read.  This is skimage.segmentation.expand_labels(mask, D) but for
 * the tie rule: scipy's distance transform gives a pixel with several nearest labels the one its scan meets first, a property of the algorithm;
 * the smallest label is a property of the data, symmetric under flips and transposition.  Integer arithmetic, no atomics: a pure function of
 * (mask, D), the same for every launch geometry and every run.  1 <= H, W, H W < 2^31, 1 <= D <= 32; labels are any positive int32.  mask, out and
 * dist2 must not overlap.  ws: ribca_expand_labels_ws_bytes(H, W, D) bytes; 0 for arguments the entry point refuses.  The piece is RESERVED: 256
 * bytes today, and the kernel neither reads nor writes it; a NULL or short workspace is refused all the same, as for every entry point that takes
 * one.  No loop of the kernel waits for another thread.  The entry point does not synchronise. */
int64_t ribca_expand_labels_ws_bytes(int32_t H, int32_t W, int32_t D);
int ribca_expand_labels(const int32_t* mask, int32_t H, int32_t W, int32_t D, int32_t* out, int32_t* dist2, void* ws, int64_t ws_bytes, void* stream);

/* ---- connected components of a mask and relabelling by component (csrc/components.hip) ------------------------------------
 * mask (H, W) int32 row-major on the device, read only; root (H, W) int32 and stats (H W, 4) int32 are OVERWRITTEN, every byte of them.
 * CLASSES: a pixel with value v > 0 belongs to class v; all pixels <= 0 form the single class "background" (negative values are background, as for
 * ribca_expand_labels).  COMPONENTS: foreground pixels of one class connect at 8-connectivity, background pixels at 4-connectivity -- the pairing
 * behind the Euler number of morphology.py, so "one component, no hole" here is euler == 1 there; pixels of different classes never connect.
 * root[p] = the raster index r W + c of the FIRST pixel of p's component, the smallest index in it: a partition of the whole image, determined
 * by the mask alone, whatever the launch geometry or the order in which threads arrive.  stats row p is meaningful where root[p] == p and 0
 * everywhere else: column 0 the area of the component; column 1 is 1 when a pixel of it lies on the image border (row 0 or H - 1, column 0 or
 * W - 1), else 0; columns 2 and 3 are lo and hi, the smallest and the largest label > 0 among the pixels that are 4-adjacent to a pixel of the
 * component and of another class, 0 and 0 when there is none.  Integer arithmetic only.  1 <= H, W, H W < 2^31; labels are any int32.  mask,
 * root, stats and ws must not overlap.  ws: ribca_mask_components_ws_bytes(H, W) bytes; 0 for arguments the entry point refuses.  The piece is
 * RESERVED: 256 bytes today, and the kernels neither read nor write it; a NULL or short workspace is refused all the same.  No loop of the
 * kernels waits for another thread.  The entry point does not synchronise.
 * ribca_mask_relabel: out[p] = new_label[root[p]] for the H W pixels; root as above (a value outside [0, H W) reads nothing and gives 0),
 * new_label (H W) int32 indexed by raster index, out (H, W) int32 OVERWRITTEN; out must not overlap root or new_label.  Same limits on H, W. */
int64_t ribca_mask_components_ws_bytes(int32_t H, int32_t W);
int ribca_mask_components(const int32_t* mask, int32_t H, int32_t W, int32_t* root, int32_t* stats, void* ws, int64_t ws_bytes, void* stream);
int ribca_mask_relabel(const int32_t* root, const int32_t* new_label, int32_t H, int32_t W, int32_t* out, void* stream);

/* ---- cell outlines: the boundary of every cell of a mask as closed rings of lattice vertices (csrc/outlines.hip) -----------
 * mask (H, W) int32 row-major on the device, read only.  LATTICE: vertex (r, c), 0 <= r <= H, 0 <= c <= W, is the top-left corner of pixel (r, c);
 * its raster index is r (W + 1) + c.  OWNERSHIP is the rule of ribca_contact_table: pixel p belongs to cell i = label_to_cell[mask[p]] when
 * 0 <= mask[p] < L and 0 <= i < n, and to no cell otherwise; nothing outside the image belongs to a cell; a label in several blobs, and several
 * labels mapped to one cell, are one cell.  BOUNDARY EDGES of cell i: every side of a pixel of i whose pixel across is not of i, as a directed
 * unit edge with the pixel on the RIGHT of the direction of travel (x = column to the right, y = row downwards): top (r, c) -> (r, c + 1), right
 * (r, c + 1) -> (r + 1, c + 1), bottom (r + 1, c + 1) -> (r + 1, c), left (r + 1, c) -> (r, c).  SUCCESSOR: where cell i has one outgoing edge
 * at the vertex an edge ends in, that edge; at a saddle -- the cell holds exactly two diagonally opposite pixels of the four around the vertex and
 * has two outgoing edges -- the LEFT turn, which joins the two pixels (the 8-connected foreground and 4-connected rest of ribca_mask_components
 * and of the Euler number of ribca_mask_morphology).  The edges of a cell fall into closed RINGS.
 * A ring row is six int64: cell; start = the raster index of the ring's smallest vertex (no two rings of one cell share it); vertices = the
 * number of vertices at which the direction changes (the start is one of them); edges = its length in unit edges; area2 = the sum over
 * consecutive kept vertices of x_k y_{k+1} - x_{k+1} y_k, positive for an exterior ring and negative for a hole; saddles = the number of times
 * the ring passes a saddle vertex.  An exterior ring leaves its start going east, a hole ring going south.
 * ribca_mask_rings: rings (cap, 6) int64 and total (1) int64 are OVERWRITTEN.  total is always the exact number of rings.  With total <= cap the
 * first total rows are the rings of the mask in an UNSPECIFIED order and every other row is -1; with total > cap only total is defined, the status
 * is still 0 and the caller calls again.  The SET of rows is a function of (mask, label_to_cell) alone, whatever the launch geometry and the order
 * in which threads arrive.  ws: ribca_mask_rings_ws_bytes(H, W, n) bytes (0 for arguments the entry point refuses): the owner of every pixel and
 * the list of candidate starts, 12 bytes per pixel.
 * ribca_mask_ring_vertices: rings (R, 6) as above in any order the caller chose; first (R + 1) int64 ascending from 0 with first[k + 1] - first[k]
 * = the vertices of row k; vertices (first[R], 2) int32 = [r, c] and bad (1) int32 are OVERWRITTEN.  Ring k is walked again from its start and
 * writes its kept vertices, the start first, in the order of the ring, at first[k].  A row that does not fit the mask -- no ring of that cell
 * starts there, the walk finds another vertex count, first[k + 1] - first[k] is not the row's count -- writes -1 into its own range
 * [first[k], first[k + 1]) and adds one to bad; a range that is none (descending, negative, past first[R]) adds one to bad and writes nothing.  No
 * thread writes outside the range of its own ring, whatever the rows say.  first lives on the device, so what is wrong with it is reported in bad,
 * not in the status.
 * Both: 1 <= H, W, (H + 1)(W + 1) < 2^31, 1 <= L, 0 <= n <= 2^21, 1 <= cap, 0 <= R; labels are any int32; integer arithmetic only.  n = 0 (and
 * R = 0) launches no walk: total = 0 and rings = -1, bad = 0.  The buffers must not overlap.  A NULL buffer, a short workspace and arguments out
 * of range are refused with a status before any HIP call.  No loop of the kernels waits for another thread, and every walk ends after at most
 * 2 (H + 1)(W + 1) steps, more than a ring has edges.  Neither entry point synchronises. */
int64_t ribca_mask_rings_ws_bytes(int32_t H, int32_t W, int32_t n);
int ribca_mask_rings(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, int64_t cap, int64_t* rings,
                     int64_t* total, void* ws, int64_t ws_bytes, void* stream);
int ribca_mask_ring_vertices(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, const int64_t* rings,
                             int32_t R, const int64_t* first, int32_t* vertices, int32_t* bad, void* stream);

/* ---- matching a second mask to the cells: the sparse contingency table of two label images (csrc/overlap.hip) -------------
 * mask_a and mask_b (H, W) int32 row-major, a_to_cell (La) int32 and b_to_obj (Lb) int32 on the device, all read only.  OWNERSHIP is the rule of
 * ribca_contact_table, applied to each mask with its own table: cell(p) = a_to_cell[mask_a[p]] when 0 <= mask_a[p] < La and the result lies in
 * [0, n), "none" otherwise; obj(p) likewise from mask_b, b_to_obj, Lb and m.  A label in several blobs is one cell (or one object).
 *     area_a[i] = #{ p : cell(p) = i }      area_b[j] = #{ p : obj(p) = j }      w(i, j) = #{ p : cell(p) = i and obj(p) = j }
 * ribca_mask_overlap: partner (n, S) int32, inter (n, S) uint64, degree (n) int32, area_a (n) int32, area_b (m) int32 and over (2) int32 are all
 * OVERWRITTEN (the library initialises them and its workspace itself).  over[0] == 0: degree[i] = the number of j with w(i, j) > 0;
 * partner[i][0 .. degree[i]) holds those j in ASCENDING order with w(i, .) beside them in inter; the rest of either row is -1 / 0; over[1] = -1.
 * over[0] > 0: that many cells overlap more than S objects, over[1] is the lowest such cell index, area_a and area_b are still exact, the other
 * outputs are unspecified -- call again with a larger S.  The result is a pure function of (mask_a, mask_b, both tables): the same for every S
 * that fits, every launch geometry and every run (integer atomics only; the rows are sorted by rank, as those of ribca_contact_table).
 * 1 <= H, W, H W < 2^31, 1 <= La, Lb, 1 <= n, m <= 2^21, S a power of two in 8 .. 1024.  ws: ribca_mask_overlap_ws_bytes(H, W, n, S) bytes, the
 * three pieces of ribca_contact_table_ws_bytes (4 n S bytes of keys, 8 n S bytes of sums, 4 n bytes of overflow flags, each rounded up to 256
 * bytes); 0 for arguments the entry point refuses.  The outputs and ws must not overlap each other or the inputs; the inputs may share memory
 * (mask_a == mask_b is allowed).
 * ribca_mask_compartments: owner (m) int32 on the device: the cell index that owns object j, or -1 (any other value owns nothing).  inner and
 * outer (H, W) int32 are OVERWRITTEN, every byte: inner[p] = mask_a[p] when cell(p) = i is a cell, obj(p) = j is an object and owner[j] == i,
 * else 0; outer[p] = mask_a[p] when cell(p) is a cell and inner[p] == 0, else 0.  inner and outer must not overlap each other or the inputs.  The
 * same limits on H, W, La, Lb, n, m; no workspace.
 * Both: a NULL buffer, sizes out of range, a NULL or short workspace and overlapping outputs are refused with a status that names the entry point,
 * before any HIP call.  No loop of any kernel waits for another thread: every probe sequence ends after at most S slots.  Neither entry point
 * synchronises. */
int64_t ribca_mask_overlap_ws_bytes(int32_t H, int32_t W, int32_t n, int32_t S);
int ribca_mask_overlap(const int32_t* mask_a, const int32_t* mask_b, int32_t H, int32_t W, const int32_t* a_to_cell, int32_t La, int32_t n,
                       const int32_t* b_to_obj, int32_t Lb, int32_t m, int32_t S, int32_t* partner, uint64_t* inter, int32_t* degree,
                       int32_t* area_a, int32_t* area_b, int32_t* over, void* ws, int64_t ws_bytes, void* stream);
int ribca_mask_compartments(const int32_t* mask_a, const int32_t* mask_b, int32_t H, int32_t W, const int32_t* a_to_cell, int32_t La, int32_t n,
                            const int32_t* b_to_obj, int32_t Lb, int32_t m, const int32_t* owner, int32_t* inner, int32_t* outer, void* stream);

/* ---- where a marker sits in the cell: depth below the cell's edge, sums per depth shell (csrc/localization.hip) ---------
 * ribca_mask_depth: mask (H, W) int32 row-major on the device, read only; depth2 (H, W) int32 is OVERWRITTEN, every byte.  With
 * l(q) = max(mask[q], 0): a pixel p with l(p) == 0 gets depth2[p] = 0.  For a pixel p with l(p) > 0 let m be the smallest squared Euclidean
 * distance from p to a pixel q INSIDE the image with l(q) != l(p) -- background or another cell, whichever is nearer: depth2[p] = m when such
 * a q exists and m <= D D, else -1, "deeper than D".  Nothing outside the image is read and nothing outside it counts as a different pixel: a
 * cell cut by the image border is measured from its VISIBLE edge only, so its pixels on the border are as deep as the rest of its outline
 * lets them be, and a label that fills the image is -1 everywhere.  Negative pixels are background, as for ribca_expand_labels.  Integer
 * arithmetic, no atomics: a pure function of (mask, D), the same for every launch geometry and every run.  1 <= H, W, H W < 2^31,
 * 1 <= D <= 32; labels are any positive int32.  mask and depth2 must not overlap.  ws: ribca_mask_depth_ws_bytes(H, W, D) bytes; 0 for
 * arguments the entry point refuses.  The piece is RESERVED: 256 bytes today, and the kernel neither reads nor writes it; a NULL or short
 * workspace is refused all the same, as for every entry point that takes one.
 * ribca_cell_shell_sums: image (C, H, W) fp32, mask and depth2 (H, W) int32, ids (n) int32 and bbox (n, 4) int32 on the device, as for
 * ribca_cell_intensities: the same clipping, the same pixel set S_i in row-major order, the same empty cases.  depth2 holds values >= -1, as
 * ribca_mask_depth writes them.  edges2 (S - 1) int32 is a HOST array, read before the launch: strictly increasing and positive,
 * 2 <= S <= 8.  THE SHELL of a pixel: S - 1 when its depth2 is -1, else #{ j : depth2 > edges2[j] }.  All three outputs are OVERWRITTEN:
 *     count   (n, S) int32      the pixels of S_i per shell
 *     deepest (n) int32         -1 when a pixel of S_i has depth2 == -1, else the largest depth2 over S_i -- the squared radius of the largest
 *                               disc centred on a pixel of the cell that holds no other pixel; 0 for a cell without a pixel
 *     sums    (n, C, S) fp64    element e of S_i is its e-th pixel in row-major order WHATEVER its shell, and belongs to partial e mod 256.
 *                               Partial p[k][j], k the shell, j = 0 .. 255, starts at 0.0 and adds, in increasing e, the values widened to
 *                               fp64 of its elements whose shell is k -- elements of other shells are skipped, not added as zeros; then for
 *                               s = 128, 64, ..., 1: p[k][j] += p[k][j+s] for j < s; the sum is p[k][0].  Every operation is rounded on
 *                               its own
 * For finite inputs the outputs are a pure function of the arguments, the same for every launch geometry and every run (no floating-point
 * atomics).  1 <= C <= 64, 1 <= H, W <= 65535, H W < 2^31, 1 <= n <= 2^21; n == 0 returns 0 and touches nothing.  No workspace.
 * Both: arguments outside the limits return a status with text (ribca_last_error) before any HIP call.  No loop of any kernel waits for
 * another thread.  Neither entry point synchronises. */
int64_t ribca_mask_depth_ws_bytes(int32_t H, int32_t W, int32_t D);
int ribca_mask_depth(const int32_t* mask, int32_t H, int32_t W, int32_t D, int32_t* depth2, void* ws, int64_t ws_bytes, void* stream);
int ribca_cell_shell_sums(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const int32_t* depth2, const int32_t* ids,
                          const int32_t* bbox, int32_t n, const int32_t* edges2, int32_t S, int32_t* count, int32_t* deepest, double* sums, void* stream);

/* ---- marker colocalisation per cell: sums, centred cross products, gated sums, counts above both gates (csrc/colocalization.hip, DESIGN.md
 * section 27) -----------------------------------------------------------------------------------------------------------------------------------
 * image (C, H, W) fp32, mask (H, W) int32, ids (n) int32 and bbox (n, 4) int32 on the device, exactly as for ribca_cell_intensities: the same
 * clipping, the same pixel set S_i -- the pixels of the clipped box with mask == ids[i] -- in row-major order, the same empty cases.  chan (K)
 * int32 and thr (K) fp32 are HOST arrays, read before the launch: chan holds K DISTINCT channel indices in [0, C), 2 <= K <= 32, in any order;
 * thr holds one finite gate per selected channel, on the image's own scale.  With a = |S_i|, v_k[e] the value of channel chan[k] at the e-th
 * pixel of S_i widened to fp64, g_k[e] the fp32 comparison value > thr[k] (STRICT; false for a NaN) and P = K (K + 1) / 2 the pairs (k, l),
 * k <= l, in the order (0,0), (0,1) .. (0,K-1), (1,1) ..., all five outputs are OVERWRITTEN:
 *     area  (n) int32        a
 *     both  (n, P) int32     #{ e : g_k[e] and g_l[e] }; the diagonal counts the pixels above the channel's own gate
 *     sums  (n, K) fp64      THE TREE over v_k: partial p_j, j = 0 .. 255, starts at 0.0 and adds v_k[j], v_k[j+256], ... in that order; then
 *                            for s = 128, 64, ..., 1: p_j += p_{j+s} for j < s; the sum is p_0.  m_k = sums / a
 *     cross (n, P) fp64      the same tree over (v_k[e] - m_k) * (v_l[e] - m_l); every operation is rounded on its own (no fused multiply-add)
 *     gated (n, K, K) fp64   gated[k][l] is the same tree over v_k[e] restricted to the elements with g_l[e]: element e belongs to partial
 *                            e mod 256 WHATEVER its gates, and an element whose gate is closed is skipped, not added as a zero -- the rule
 *                            of ribca_cell_shell_sums
 * Two consequences.  sums[i][k] and cross[i][(k, k)] equal the sum and the ssd ribca_cell_intensities gives channel chan[k], bit for bit.  A
 * channel that is constant over the cell gives cross of exactly 0.0 in its row and column: the sum of a equal fp32 values is exact in fp64
 * (a < 2^31, 24-bit significands), and so is its quotient by a, so every deviation is 0.0.
 * a = 0 gives zeros everywhere.  For finite inputs the outputs are a pure function of the arguments, the same for every launch geometry and
 * every run (no floating-point atomics; the counts are integer adds); for non-finite values only area and both are specified.
 * 1 <= C <= 64, 2 <= K <= 32, 1 <= H, W <= 65535, H W < 2^31, 1 <= n <= 2^21; n == 0 returns 0 and touches nothing.  A NULL buffer, sizes out
 * of range, a repeated or out-of-range chan and a non-finite thr are refused with a status that names the entry point (ribca_last_error)
 * before any HIP call.  No workspace.  No loop of the kernel waits for another thread.  The entry point does not synchronise. */
int ribca_cell_coloc(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const int32_t* ids, const int32_t* bbox, int32_t n,
                     const int32_t* chan, const float* thr, int32_t K, int32_t* area, int32_t* both, double* sums, double* cross, double* gated,
                     void* stream);

/* Neighbourhood compositions of spatial_methods.tissue_region_partition (spatial_methods.py:133-180): sizes (DEVICE array, n_sizes <= 8,
 * strictly increasing, max <= 255; the reference uses 10,20,30,50,75,100,150,200; n_types <= 254) -> counts (n_cells, n_sizes, n_types) uint16 =
 * number of cells of each type among the nearest sizes[l] OTHER cells (fp64 distances, ties towards the lower index).  The
 * reference divides each row by its sum and feeds PCA + KMeans on the host.  Synchronises the stream once (reads sizes). */
int ribca_knn_compositions(const double* x, const double* y, const int32_t* cell_type, int32_t n_cells, int32_t n_types, const int32_t* sizes,
                           int32_t n_sizes, uint16_t* counts, void* stream);

/* ---- tissue regions (spatial_methods.tissue_region_partition, spatial_methods.py:133-198: PCA(0.99) + KMeans of the composition table on the
 * host, unseeded).  csrc/regions.hip; scikit-learn 1.7's defaults restated and seeded, DESIGN.md section 11.  All arithmetic is fixed so that a
 * numpy loop reproduces it bit for bit: integer sums for the PCA statistics, fp64 sums in a stated order with no fma contraction elsewhere, no
 * float atomics.  Supported range, everywhere below: n >= 1, 1 <= F <= 2032 (8 sizes x 254 types), 1 <= d <= 2032, 1 <= k <= min(n, 256);
 * outside it an entry point returns 1 with a text. */

/* counts (n, F) int16 = the output of ribca_knn_compositions seen as n rows of F = n_sizes * n_types columns, every count in 0 .. 255 (else an
 * error): colsum (F) int64 = column sums, gram (F, F) int64 = counts^T counts -- exact, whatever the launch geometry.  Both are overwritten.
 * ws: ribca_region_gram_ws_bytes(n, F) bytes.  Synchronises the stream once (reads the range flag). */
int64_t ribca_region_gram_ws_bytes(int32_t n, int32_t F);
int ribca_region_gram(const int16_t* counts, int32_t n, int32_t F, int64_t* colsum, int64_t* gram, void* ws, int64_t ws_bytes, void* stream);

/* y (n, d) fp64: y[i, j] = sum over f = 0 .. F - 1, in that order, of (counts[i, f] / size_col[f] - mean[f]) * comps[j, f]; size_col, mean (F)
 * and comps (d, F) fp64.  The fp64 composition table is never formed.  d <= F. */
int ribca_region_project(const int16_t* counts, int32_t n, int32_t F, const double* size_col, const double* mean, const double* comps, int32_t d,
                         double* y, void* stream);

/* One k-means++ step: for each of the n_cand <= 8 candidate rows cand[t] of y (n, d) fp64, cand_d2[t, i] = min(closest[i], d2(i, cand[t]))
 * (closest NULL = no minimum yet) with d2 = the fp64 sum of squared differences in dimension order, and pot[t] = the sum of cand_d2[t, :]
 * taken as: rows of every chunk of 1024 in ascending order, then the chunks in ascending order.  ws: ribca_kmeans_trials_ws_bytes(n, n_cand)
 * bytes (the query sees n and n_cand only: it is 0 where they are out of range, not where d is). */
int64_t ribca_kmeans_trials_ws_bytes(int32_t n, int32_t n_cand);
int ribca_kmeans_trials(const double* y, int32_t n, int32_t d, const int32_t* cand, int32_t n_cand, const double* closest, double* cand_d2,
                        double* pot, void* ws, int64_t ws_bytes, void* stream);

/* labels[i] = the j with the least (d2(i, centres[j]), j); mind2 (n, optional) = that d2; changed[0] (uint32) = number of rows whose label
 * differs from the one labels held on entry. */
int ribca_kmeans_assign(const double* y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, double* mind2, uint32_t* changed,
                        void* stream);

/* The M step.  sums (k, d) fp64 and counts (k) int32: per (cluster, dimension) the rows of every chunk of 1024 added in ascending order, then the
 * chunks added in ascending order.  Then ribca_kmeans_finalize.  ws: ribca_kmeans_update_ws_bytes(n, d, k) bytes. */
int64_t ribca_kmeans_update_ws_bytes(int32_t n, int32_t d, int32_t k);
int ribca_kmeans_update(const double* y, int32_t n, int32_t d, const int32_t* labels, int32_t k, const double* centres_old, double* centres_new,
                        double* sums, int32_t* counts, const uint32_t* changed, double* stat, void* ws, int64_t ws_bytes, void* stream);
/* centres_new = sums / counts (the old centre where a count is 0); stat (1 + 2 k) fp64: [0] = changed[0] (0 if NULL), [1 + j] = counts[j],
 * [1 + k + j] = sum over the dimensions in ascending order of (centres_new[j, f] - centres_old[j, f])^2.  What the host reads per iteration. */
int ribca_kmeans_finalize(const double* sums, const int32_t* counts, int32_t k, int32_t d, const double* centres_old, double* centres_new,
                          const uint32_t* changed, double* stat, void* stream);
/* scikit-learn's rule for empty clusters, on the sums: for m = 0 .. n_empty - 1 in order, row far_rows[m] is subtracted from the sum of its
 * cluster (labels[far_rows[m]], count - 1) and becomes the sum of cluster empty_ids[m] (count 1).  Call ribca_kmeans_finalize afterwards. */
int ribca_kmeans_relocate(const double* y, int32_t n, int32_t d, int32_t k, const int32_t* labels, const int32_t* far_rows, const int32_t* empty_ids,
                          int32_t n_empty, double* sums, int32_t* counts, void* stream);

/* ---- extra cell types (Annotator._find_extra_cell_types, model.py:642-675: umap.UMAP(n_components=5).fit_transform of the intensity rows
 * of every "Others" cell, then HDBSCAN).  umap-learn 0.5's fit_transform and sklearn's HDBSCAN defaults restated; DESIGN.md section
 * "Extra cell types". */

/* Exact k nearest rows of x (n, dim) fp32, the row itself included: idx (n, k) int32 and dist (n, k) fp32, each row sorted by (distance,
 * index).  A distance is sqrt of the fp32 sum of squared differences taken in dimension order (no |x|^2 + |y|^2 - 2 x.y expansion).
 * k <= min(n, 64), dim <= 256. */
int ribca_knn_dense(const float* x, int32_t n, int32_t dim, int32_t k, int32_t* idx, float* dist, void* stream);

/* umap's smooth_knn_dist (local_connectivity 1, bandwidth 1, target log2(k) over neighbours 1..k-1, 64 bisection steps, tolerance 1e-5,
 * floor 1e-3 x the row mean -- the mean of all n k distances for a row without a positive distance) and compute_membership_strengths over
 * the output of ribca_knn_dense: sigma (n), rho (n), w (n, k) fp32 with w = 0 for the row itself, 1 where d - rho <= 0, else
 * exp(-(d - rho) / sigma).  2 <= k <= 64. */
int ribca_umap_fuzzy_weights(const int32_t* idx, const float* dist, int32_t n, int32_t k, float* sigma, float* rho, float* w, void* stream);

/* n_epochs epochs of umap's optimize_layout_euclidean (move_other) on emb (n, dim) fp32 in place, dim <= 8.  The graph is symmetric CSR:
 * indptr (n + 1) int64, indices (nnz) int32, rev (nnz) int64 = position of edge (k, j) for edge (j, k), eps (nnz) fp64 = epochs_per_sample.
 * Two deliberate deviations from umap: every epoch is a Jacobi step (each vertex sums its out-edge and negative-sample forces, then the
 * move_other terms of its in-edges, in CSR order, and all vertices move after the epoch: no atomics, bit-reproducible), and negative
 * sample p of edge e in epoch t is a counter-based hash of (seed, t, e, p) mod n.  ws: device workspace of at least
 * ribca_umap_optimize_ws_bytes(n, dim, nnz) bytes.  Synchronises the stream once (reads indptr[n]). */
int64_t ribca_umap_optimize_ws_bytes(int32_t n, int32_t dim, int64_t nnz);
int ribca_umap_optimize(float* emb, int32_t n, int32_t dim, const int64_t* indptr, const int32_t* indices, const int64_t* rev, const double* eps,
                        double a, double b, double gamma, double alpha0, double neg_rate, int32_t n_epochs, uint64_t seed, void* ws,
                        int64_t ws_bytes, void* stream);

/* HDBSCAN* on dense fp32 points, the O(n^2) part (csrc/hdbscan.hip; the tree part after the spanning tree is host code, manifold.py).  The
 * arithmetic is fixed so that a numpy loop reproduces it bit for bit: d2(i, j) = fp32 sum of squared differences in dimension order (no fma
 * contraction, as in ribca_knn_dense); every comparison is made on squared values.
 *
 * core2 (n) fp32 = the min_samples-th smallest d2(i, .) with the point itself counted (sklearn's kneighbors(X, min_samples)[:, -1], squared).
 * n >= 2, 1 <= dim <= 64, 1 <= min_samples <= n (up to 64 a sorted list in registers, above that a bisection on the bit pattern of d2 with
 * one counting pass per step: no per-row list).  ws: ribca_core_distance_ws_bytes(n, dim, min_samples) bytes.  Synchronises the stream once; a
 * core distance that is not finite (NaN or infinite coordinates) is an error. */
int64_t ribca_core_distance_ws_bytes(int32_t n, int32_t dim, int32_t min_samples);
int ribca_core_distance(const float* x, int32_t n, int32_t dim, int32_t min_samples, float* core2, void* ws, int64_t ws_bytes, void* stream);

/* The minimum spanning tree of the mutual-reachability graph, mreach2(i, j) = max(core2(i), core2(j), d2(i, j)), under the total order
 * (mreach2, min(i, j), max(i, j)) -- under it the tree is unique, so the result does not depend on the launch geometry: n - 1 edges with
 * edges_u < edges_v (int32) and edges_w = sqrt(mreach2) (fp32), in an unspecified but reproducible order.  Boruvka rounds (at most
 * ceil(log2 n)); the n x n matrix is never formed.  n >= 2, 1 <= dim <= 64.  ws: device workspace of at least ribca_mreach_mst_ws_bytes(n)
 * bytes.  Synchronises the stream once per round (reads the number of components left); a negative or non-finite core distance is an error. */
int64_t ribca_mreach_mst_ws_bytes(int32_t n);
int ribca_mreach_mst(const float* x, int32_t n, int32_t dim, const float* core2, int32_t* edges_u, int32_t* edges_v, float* edges_w, void* ws,
                     int64_t ws_bytes, void* stream);

/* ---- spectral start of the embedding on the GPU (umap's spectral_layout; csrc/spectral.hip).  The three operations of a
 * block eigensolver that touch all n rows; the solver itself (manifold.spectral_component_gpu) is host code over them.  All fp64, every
 * product and sum rounded on its own, the order of every sum fixed: a numpy loop reproduces each bit (tests/spectral_numpy.py). */

/* y = alpha (S x) + beta x + gamma z, S = D^-1/2 A D^-1/2: A the symmetric canonical CSR graph of ribca_umap_optimize (indptr (n + 1) int64,
 * indices (nnz) int32, weights (nnz) fp32), dinv (n) fp64 = 1 / sqrt(degree); x, y, z (n, m) row-major fp64, 1 <= m <= 16.
 * (S x)[i, c] = the sum, started at 0, over the entries e of row i in CSR order of ((dinv[i] * (double) w[e]) * dinv[j_e]) * x[j_e, c]; then
 * v = alpha * that; v = v + beta * x[i, c] unless beta == 0; v = v + gamma * z[i, c] unless z is NULL.  A row without entries gives
 * beta x + gamma z.  y must not be x; y may be z.  Entries outside [0, nnz) and columns outside [0, n) are skipped, never read. */
int ribca_spectral_spmm(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t nnz, const double* dinv, int32_t n, int32_t m,
                        const double* x, double alpha, double beta, double gamma, const double* z, double* y, void* stream);

/* g (p, q) = u^T v for u (n, p), v (n, q) fp64, p, q <= 48: per output the rows of every chunk of 1024 added in ascending order (started at 0),
 * then the chunks added in ascending order (started at 0).  ws: ribca_spectral_gram_ws_bytes(n, p, q) = 8 p q ceil(n / 1024) bytes. */
int64_t ribca_spectral_gram_ws_bytes(int32_t n, int32_t p, int32_t q);
int ribca_spectral_gram(const double* u, const double* v, int32_t n, int32_t p, int32_t q, double* g, void* ws, int64_t ws_bytes, void* stream);

/* x (n, m) = u (n, p) c (p, m), p, m <= 48: x[i, j] = (x[i, j] if add, else 0) + u[i, 0] * c[0, j] + ... + u[i, p - 1] * c[p - 1, j], added in
 * that order.  x must not be u. */
int ribca_spectral_combine(const double* u, int32_t n, int32_t p, const double* c, int32_t m, int32_t add, double* x, void* stream);

/* ---- scatter plot (Annotator.umap_visualization, model.py:746-765; csrc/scatter.hip) ---------------------------------------------------
 * points (n, 2) fp32, rgb (n, 3) uint8 -> out (height, width, 3) uint8, white background.  Point i has its centre at column
 * rint(x * (float) ax + (float) bx), row rint(y * (float) ay + (float) by) (fp32, no contraction) and covers the pixels at offsets (dx, dy) with
 * dx^2 + dy^2 <= radius^2 + 1 (|dx|, |dy| <= radius <= 16) that lie on the canvas; where discs overlap the point with the highest index
 * shows (integer atomicMax: reproducible bytes).  A centre that is not finite or not on the canvas is skipped; *skipped (HOST) = how many.
 * ws: ribca_scatter_raster_ws_bytes(height, width) bytes.  height, width <= 16384.  Synchronises the stream once. */
int64_t ribca_scatter_raster_ws_bytes(int32_t height, int32_t width);
int ribca_scatter_raster(const float* points, const uint8_t* rgb, int32_t n, double ax, double bx, double ay, double by, int32_t height, int32_t width,
                         int32_t radius, uint8_t* out, int64_t* skipped, void* ws, int64_t ws_bytes, void* stream);

/* ---- per-cell-type statistics and their plots (Annotator.generate_heatmap, model.py:700-741; Annotator.cell_type_composition,
 * model.py:861-912; csrc/celltype_stats.hip) -------------------------------------------------------------------------------------------------
 * ribca_group_sums: x (n, c) fp64 row-major, group (n) int32 -> sums (groups, c) fp64, counts (groups) int64 (device), *skipped (HOST) = the rows
 * whose id lies outside [0, groups): they are ignored, which is how a caller masks rows.  Sums and counts, not means: partial results of several
 * images or ranks combine exactly in the counts and in an order the caller fixes in the sums.  1 <= c <= 1024, 1 <= groups <= 256,
 * 0 <= n < 2^31 - 1; n = 0 gives zeros.  sums is a pure function of x and group -- no floating-point atomic; it does not depend on the launch
 * geometry, the device, the workspace or the stream -- with THE summation tree, every addition rounded on its own (no fma), R = 1024:
 *     chunk k = the rows [k R, min(n, (k + 1) R));  part[k][g][j] = (((+0.0 + x[r0][j]) + x[r1][j]) + ...) over the rows r0 < r1 < ... of chunk k
 *     whose id is g (+0.0 when there is none);  sums[g][j] = (((+0.0 + part[0][g][j]) + part[1][g][j]) + ...) over ALL chunks in ascending k.
 * In numpy:  part = np.zeros((chunks, groups, c));  for r in range(n): part[r // 1024, group[r]] += x[r]  (ids in range only);
 *            sums = np.zeros((groups, c));  for k in range(chunks): sums += part[k].
 * ws: ribca_group_sums_ws_bytes(n, c, groups) bytes (0 for arguments the entry point refuses).  Synchronises the stream once. */
int64_t ribca_group_sums_ws_bytes(int32_t n, int32_t c, int32_t groups);
int ribca_group_sums(const double* x, const int32_t* group, int32_t n, int32_t c, int32_t groups, double* sums, int64_t* counts, int64_t* skipped,
                     void* ws, int64_t ws_bytes, void* stream);
/* ribca_heatmap_raster: sums (rows, cols) fp64, counts (rows) int64, lut (256, 3) uint8 -> out (rows cell, cols cell, 3) uint8 and *vmin, *vmax
 * (HOST).  mean = sums[t][j] / (double) counts[t], NaN where counts[t] <= 0; vmin / vmax = the smallest / largest mean that is not NaN (NaN when
 * there is none: numpy's nanmin / nanmax, seaborn's default).  The pixel (y, x) belongs to the table cell (y / cell, x / cell); it is white
 * (255) when y % cell or x % cell lies outside [gap, cell - gap), silver (192) when the mean is NaN, and otherwise lut[i] with i = 0 when
 * vmax == vmin, else q = floor(((mean - vmin) / (vmax - vmin)) * 256.0), every operation rounded on its own, i = 255 when q >= 255, (int) q when
 * 0 <= q < 255, 0 otherwise.  1 <= rows <= 256, 1 <= cols <= 1024, 1 <= cell <= 64, 0 <= 2 gap < cell.
 * ws: ribca_heatmap_raster_ws_bytes(rows, cols, cell, gap) bytes.  Synchronises the stream once. */
int64_t ribca_heatmap_raster_ws_bytes(int32_t rows, int32_t cols, int32_t cell, int32_t gap);
int ribca_heatmap_raster(const double* sums, const int64_t* counts, int32_t rows, int32_t cols, const uint8_t* lut, int32_t cell, int32_t gap, uint8_t* out,
                         double* vmin, double* vmax, void* ws, int64_t ws_bytes, void* stream);
/* ribca_table_raster: values (rows, cols) fp64 -> out (rows cell, cols cell, 3) uint8 on a colour scale the CALLER gives: geometry, gap and index
 * rule of ribca_heatmap_raster with vmin, vmax as arguments and the value clamped to [vmin, vmax] first; silver where the value is NaN; lut[128]
 * for every number when vmax == vmin.  vmin <= vmax, both finite; the limits of ribca_heatmap_raster.  No workspace; does not synchronise. */
int ribca_table_raster(const double* values, int32_t rows, int32_t cols, const uint8_t* lut, int32_t cell, int32_t gap, double vmin, double vmax,
                       uint8_t* out, void* stream);
/* ribca_pie_raster: rays (m, 2) fp64 = (cos, sin) of the m interior wedge boundaries in ascending angle, rgb (m + 1, 3) uint8 -> out (size, size, 3)
 * uint8.  The centre is the pixel (size / 2, size / 2); a pixel at the integer offset v = (dx to the right, dy UPWARDS) with
 * dx^2 + dy^2 <= radius^2 gets rgb[w], w = the number of rays a for which NOT (v < a); every other pixel is white.  The order of directions is that
 * of their angles in [0, 2 pi) from 3 o'clock, counter-clockwise on screen (matplotlib's ax.pie), decided without a transcendental:
 *     half(u) = 0 if (u.y > 0 or (u.y == 0 and u.x > 0)) else 1;   u < a  iff  half(u) < half(a), or half(u) == half(a) and u.x * a.y - u.y * a.x > 0
 * (fp64, the two products and the difference rounded on their own).  The centre pixel gets rgb[0].  m = 0: a disc of rgb[0].
 * 0 <= m <= 256, 1 <= size <= 16384, 0 <= radius <= size.  No workspace; does not synchronise. */
int ribca_pie_raster(const double* rays, int32_t m, const uint8_t* rgb, int32_t size, int32_t radius, uint8_t* out, void* stream);

/* ---- vote (Annotator.merge_by_voting, model.py:481-633) ------------------------------------------------------ */
/* Global class ids: 0..16 = key order of utils.get_void_vote (utils.py:143-146), 17 = "Others".
 * p_a (n, k_a) and optional p_b (n, k_b) are softmax outputs; map_* (k) int8 give each class's global id;
 * type_conf (18) fp32 per-type thresholds (negative = unset); label (n) int8 and conf (n) fp32 (-1 = thresholded). */
int ribca_vote(const float* p_a, int32_t k_a, const int8_t* map_a, const float* p_b, int32_t k_b, const int8_t* map_b,
               const float* type_conf, float conf, int32_t n, int8_t* label, float* out_conf, void* stream);

/* ---- profiling (kernel-level test hooks: include/ribca_hip_test.h, a library of their own) ------------------------- */
/* When enabled, every kernel launch of the ViT forward is bracketed by HIP events on its stream; ribca_prof_read
 * synchronises and returns, per kernel class, total milliseconds and launch count since the last reset.
 * classes: 0 gemm_qkv 1 gemm_proj 2 gemm_fc1 3 gemm_fc2 4 gemm_embed 5 attention 6 layernorm (row statistics) 7 cell_qkv_attention
 * (the per-cell fused norm1 -> qkv -> attention kernel of D <= 384) 8 head 9 other */
int ribca_prof_enable(int32_t on);
int ribca_prof_read(double* ms_out10, int64_t* count_out10);
const char* ribca_prof_name(int32_t cls);

/* NOT part of the stable ABI.  The versioned table of host launchers that libribca_hip_test.so (the kernel-level hooks of tests/ and tools/,
 * include/ribca_hip_test.h) binds instead of C++ symbols: csrc/ribca_internal.h describes it and belongs to one build.  NULL for any other
 * version than that build's RIBCA_INTERNAL_VERSION.  A caller of the product ABI never needs it. */
const void* ribca_internal_table(int32_t version);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* RIBCA_HIP_H */
