/*
 * codenerf.h — C ABI of libcodenerf_hip.so, the MI355X (gfx950) Code-NeRF renderer.
 *
 * Drop-in boundary for the ray-marching hot path of akashsharma02/code-nerf.
 * The reference is pure Python (PyTorch 1.8) with no FFI; each entry point
 * below replaces one of its tensor-in/tensor-out functions (cited file:line,
 * relative to the reference root).  The Python mirror (code-nerf_amd/codenerf)
 * binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions (all entry points):
 *   - Pointers are DEVICE pointers to contiguous row-major fp32 (int64 for
 *     indices) unless marked "host".  The caller owns every buffer; nothing
 *     is allocated, freed or retained across calls.
 *   - Work is enqueued on `stream` (a hipStream_t; NULL = legacy default
 *     stream) and is asynchronous; no entry point synchronises the device,
 *     so all of them can be captured into a hipGraph.
 *   - Return value: 0 on success; a negative CN_E* for an argument error
 *     (nothing launched); a positive hipError_t from the launch.
 *   - Reentrant; one process per GPU (mirrors mp.spawn in train.py/eval.py).
 *   - Buffer contract.  An output is WRITTEN (every documented element stored, whatever it held) or
 *     ACCUMULATED (added to what the caller put there: zeros, or a running sum).  A `workspace` is
 *     scratch: its contents on entry are ignored -- it may hold anything, NaNs included -- unless the
 *     entry says which earlier call must have filled it.  No entry point stores outside the
 *     documented extent of a buffer, and a strided output (ldc > row length) keeps its gap columns.
 *     tests/buffers.py makes this executable (NaN-poisoned allocations, trailing guards).
 */
#ifndef CODENERF_H_
#define CODENERF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cn_stream_t; /* hipStream_t */

#define CN_OK 0
#define CN_EINVAL (-1)       /* bad size / null pointer / out-of-range argument */
#define CN_EUNSUPPORTED (-2) /* configuration outside what the kernels implement */

/* Architecture the fused MLP kernels implement (CodeNeRFModel, model.py:123-158,
 * as every runnable config instantiates it: hidden_size 256, code sizes 256,
 * num_encoding_fn_xyz 10, num_encoding_fn_dir 4, include_input_* True). */
#define CN_HIDDEN 256
#define CN_CODE 256
#define CN_DIM_XYZ 63
#define CN_DIM_DIR 27
#define CN_NUM_PARAMS 18        /* weight/bias tensors of CodeNeRFModel, state_dict order */
#define CN_CODE_BIAS_STRIDE 520 /* floats per code row: c_xyz2[256] c_feat[256] c_sigma c_rgb[3] pad[4] */

/* Packed-weight formats of the field kernel (cn_mlp_pack):
 *   CN_FMT_F32    fp32 fragments, v_mfma_f32_32x32x2_f32 (exact f32 products);
 *   CN_FMT_BF16X3 bf16 hi/lo fragments, Wh.Xh + Wh.Xl + Wl.Xh on
 *                 v_mfma_f32_32x32x16_bf16 with fp32 accumulation (~2^-17 relative
 *                 per product; 5.3x the fp32 MFMA rate). */
#define CN_FMT_F32 0
#define CN_FMT_BF16X3 1
/*   CN_FMT_BF16X3_T  the transposed 3xbf16 pack the fused backward streams
 *                    (cn_field_backward_x3); not a forward format. */
#define CN_FMT_BF16X3_T 2
/*   CN_FMT_F32_W16   fp32 fragments for v_mfma_f32_16x16x4_f32 at two waves per SIMD
 *                    (the inference kernel of precision "f32"; exact f32 products as
 *                    CN_FMT_F32, whose kernel remains the training forward). */
#define CN_FMT_F32_W16 3
/*   CN_FMT_F32_W16_T the transposed fp32 pack the fused fp32 backward streams
 *                    (cn_field_backward_fused); not a forward format. */
#define CN_FMT_F32_W16_T 4
/*   CN_FMT_BF16X3_W16 the same 3-product bf16 split as CN_FMT_BF16X3 on
 *                    v_mfma_f32_16x16x32_bf16 at two waves per SIMD (16 samples per wave;
 *                    cn_mlp_forward / cn_radiance_field only -- the mask-writing forward and
 *                    the fused backward take CN_FMT_BF16X3 / _T). */
#define CN_FMT_BF16X3_W16 5
/*   CN_FMT_F32_W16_FOLD the CN_FMT_F32_W16 pack for inference with frozen weights, with fc_out's 256
 *                    feature rows folded into layer_dir1 (model.py:186-189 has no activation between
 *                    them): W_f = W_dir1[:, :256] W_out[1:, :256], each element a 256-term dot product
 *                    accumulated in double and rounded once.  28 weight chunks per tile instead of
 *                    36 (xyz1 2 | xyz2 8 | view-dir 1 | fold 8 | dir2 8 | rgb 1: the view-direction
 *                    chunk before W_f's, so what it adds depends on the ray alone and cn_view_rows can
 *                    tabulate it), 441,344 instead of 572,416 FLOP per sample; sigma_raw has
 *                    CN_FMT_F32_W16's bits.  Read by cn_mlp_forward_fold / cn_radiance_field_fold /
 *                    cn_view_rows / cn_radiance_field_fold_rows only, with cn_fold_bias's rows; every
 *                    other entry point returns CN_EUNSUPPORTED for it.  No training or backward form
 *                    (their gradients need feat and fc_out's input gradient). */
#define CN_FMT_F32_W16_FOLD 6
/*   CN_FMT_F16       fp16 fragments, one product per GEMM on v_mfma_f32_32x32x16_f16 with fp32
 *                    accumulation: the opt-in fast inference kernel (precision "f16"), NOT the
 *                    reference's arithmetic.  The rule (tests/field_f16_cases.py states it in float64):
 *                      - the six GEMM weight matrices -- layer_xyz1, layer_xyz2[:, :256],
 *                        fc_out[1:, :256], layer_dir1, layer_dir2, fc_rgb[:, :256] -- are rounded to
 *                        fp16, round to nearest even, once at pack time;
 *                      - every vector an MFMA reads -- the 63 position encodings, h1, h2, feat, the 27
 *                        view encodings, v1, v2 -- is rounded to fp16 (RNE) where it is read; a value
 *                        beyond the fp16 range becomes +-inf;
 *                      - everything else is fp32 and unrounded: the encodings' own arithmetic, every
 *                        bias (the accumulators start from the fp32 values), the per-code terms of
 *                        cn_code_bias (unchanged, stride CN_CODE_BIAS_STRIDE) and the accumulation,
 *                        whose order is not specified;
 *                      - sigma_raw (fc_out row 0) is an fp32 dot product of the fp32 weights with the
 *                        unrounded h2, plus its per-code term, in every input mode;
 *                      - ReLU is max(x, 0) with a NaN giving 0 (v_max_f32).
 *                    The pack holds the fp16 fragments (36 chunks of 16 KiB) and 1024 fp32 constants in
 *                    a float buffer of cn_mlp_packed_floats(CN_FMT_F16) floats.  cn_mlp_forward and
 *                    cn_radiance_field run it in all their forms; it has no mask, training, backward,
 *                    density, counted or folded form: those entries refuse it as they refuse
 *                    CN_FMT_BF16X3_W16. */
#define CN_FMT_F16 7

const char* cn_version(void);
const char* cn_error_string(int code);

/* --- Rays: view_synthesis/nerf/ray_sampler.py -------------------------- */

/* RaySampler.__init__ directions, ray_sampler.py:35-51 (Q3: no +0.5).
 * dirs: (height, width, 3). */
int cn_ray_directions(int64_t height, int64_t width, float focal, float cx, float cy,
                      float* dirs, cn_stream_t stream);

/* RaySampler.get_bundle, ray_sampler.py:84-99: rd = R * d, ro = t.
 * dirs: (hw, 3); c2w: (batch, 4, 4); ro, rd: (batch, hw, 3). */
int cn_ray_bundle(const float* dirs, int64_t hw, const float* c2w, int64_t batch,
                  float* ro, float* rd, cn_stream_t stream);

/* RaySampler.sample gather, ray_sampler.py:77-80 (indices from the host RNG).
 * ro, rd: (batch, hw, 3); select_inds: (batch, sample_size) int64;
 * ro_out, rd_out: (batch*sample_size, 3). */
int cn_gather_rays(const float* ro, const float* rd, int64_t batch, int64_t hw,
                   const int64_t* select_inds, int64_t sample_size, float* ro_out,
                   float* rd_out, cn_stream_t stream);

/* --- Fused pose path (eval.py:22-38 pose_spherical + ray_sampler.py:53-99 sample
 *     + eval.py:147-148 target gather) ------------------- */

/* The pose from theta, phi, rho (batch) each (eval.py:33-37), or given as c2w (batch, 4, 4)
 * when theta is NULL, then ONLY the selected rays:
 * select_inds (batch, sample_size) int64 (the sample gather, ray_sampler.py:77-80), or NULL
 * with sample_size == hw for the whole bundle (get_bundle).  dirs: (hw, 3) from
 * cn_ray_directions.  ro, rd: (batch*sample_size, 3); c2w_out (batch, 4, 4) or NULL;
 * target (batch, hw, target_channels) gathered into target_out (batch*sample_size,
 * target_channels) when both are non-NULL.  Out-of-range indices give NaN rows. */
int cn_pose_rays(const float* theta, const float* phi, const float* rho, const float* c2w, int64_t batch,
                 const float* dirs,
                 int64_t hw, const int64_t* select_inds, int64_t sample_size, const float* target,
                 int64_t target_channels, float* c2w_out, float* ro, float* rd, float* target_out,
                 cn_stream_t stream);

/* Backward of cn_pose_rays from g_ro / g_rd (batch*sample_size, 3; either may be NULL, not
 * both): d_c2w (batch, 4, 4) WRITTEN (rows 0..2; row 3 zero) and/or d_theta, d_phi, d_rho
 * (batch) WRITTEN (any may be NULL) through the analytic d c2w / d(theta, phi, rho). */
int cn_pose_rays_backward(const float* theta, const float* phi, const float* rho, int64_t batch,
                          const float* dirs, int64_t hw, const int64_t* select_inds, int64_t sample_size,
                          const float* g_ro, const float* g_rd, float* d_c2w, float* d_theta, float* d_phi,
                          float* d_rho, cn_stream_t stream);

/* Device replacement of ray_sampler.py:41-42's np.random.permutation(hw)[:sample_size]
 * per image (throughput mode; same distribution, not the same draws): Philox4x32-10 keyed
 * by seed, counter (pixel, image, offset).  select_inds: (batch, sample_size) int64.
 * hw <= 16384 (one workgroup sorts an image's keys in LDS), else CN_EUNSUPPORTED. */
int cn_random_select(int64_t batch, int64_t hw, int64_t sample_size, uint64_t seed, uint64_t offset,
                     int64_t* select_inds, cn_stream_t stream);

/* The eval pose metric, eval.py:161-162: twist = SE3.Log(inverse(gt) @ cam)
 * (utils/lieutils.py:709-718) and err = ||twist||_2 per pose.  gt_c2w, cam_c2w: (batch, 4, 4);
 * twist (batch, 6) = (w, v) and/or err (batch). */
int cn_pose_error(const float* gt_c2w, const float* cam_c2w, int64_t batch, float* twist, float* err,
                  cn_stream_t stream);

/* --- SRN data resident in HBM (view_synthesis/datasets/dataset.py:60-94) --
 * images: (n_views, hw, channels) uint8, the decoded and cropped views; view_index: (batch) int64.
 * color (batch, hw, channels) = u8 / 255.0 (rounded once to fp32, as numpy's float64 quotient
 * cast to float32) and/or mask (batch, hw) = 1.0 where every channel != 255, else 0.0. */
int cn_srn_unpack(const uint8_t* images, int64_t n_views, int64_t hw, int64_t channels,
                  const int64_t* view_index, int64_t batch, float* color, float* mask, cn_stream_t stream);

/* --- Points: view_synthesis/nerf/point_sampler.py ---------------------- */

/* PointSampler.sample_uniform, point_sampler.py:49-71.
 * z_bins/lower/upper: (nc) from PointSampler.__init__ (:33-47);
 * t_rand: (n_rays, nc) or NULL (no perturbation);
 * z_out: (n_rays, nc); pts_out: (n_rays, nc, 3) or NULL. */
int cn_sample_uniform(const float* ro, const float* rd, int64_t n_rays, const float* z_bins,
                      const float* lower, const float* upper, int64_t nc, const float* t_rand,
                      float* z_out, float* pts_out, cn_stream_t stream);

/* pts = ro + rd * z for per-ray depth lists (point_sampler.py:70 and :118).
 * ro, rd: (n_rays, 3); z: (n_rays, n_samples); pts: (n_rays, n_samples, 3). */
int cn_ray_points(const float* ro, const float* rd, const float* z, int64_t n_rays,
                  int64_t n_samples, float* pts, cn_stream_t stream);

/* PointSampler.sample_pdf, point_sampler.py:73-120.
 * weights: row r at weights + r*w_stride, nc-2 values (the coarse weights[..., 1:-1]);
 * z: (n_rays, nc) sorted; u: row r at u + r*u_stride, nf values (u_stride 0 = one
 * row for every ray, e.g. the host's torch.linspace(0, 1, nf)), or NULL for an
 * in-kernel linspace;
 * z_out: (n_rays, nc+nf) sorted; pts_out: (n_rays, nc+nf, 3) or NULL.  nc <= 256, nf <= 256. */
int cn_sample_pdf(const float* ro, const float* rd, const float* weights, int64_t w_stride,
                  const float* z, int64_t n_rays, int64_t nc, int64_t nf, const float* u,
                  int64_t u_stride, float* z_out, float* pts_out, cn_stream_t stream);

/* --- Encoding: view_synthesis/nerf/position_embed.py ------------------- */

/* PositionalEmbedder.embed, position_embed.py:35-53.
 * x: (m, d); freqs: HOST array of num_freq floats (frequency_bands, :17-33);
 * out: (m, d*(include_input + 2*num_freq)).  num_freq <= 32. */
int cn_posenc(const float* x, int64_t m, int64_t d, const float* freqs, int64_t num_freq,
              int include_input, float* out, cn_stream_t stream);

/* --- Volume integration: view_synthesis/nerf/volumetric_render.py ------ */

/* volume_render, volumetric_render.py:36-66.
 * raw: (n_rays, n_samples, 4); z: (n_rays, n_samples); rd: (n_rays, 3);
 * rgb: (n_rays, 3); disp, acc, depth: (n_rays); weights: (n_rays, n_samples) or NULL.
 * raw, z and weights are read / written with 16-B vector accesses: 16-B aligned, or CN_EINVAL. */
int cn_volume_render(const float* raw, const float* z, const float* rd, int64_t n_rays,
                     int64_t n_samples, float* rgb, float* disp, float* acc, float* weights,
                     float* depth, cn_stream_t stream);

/* --- Code-conditioned MLP: view_synthesis/models/model.py -------------- */

/* Every field entry point below stores raw / reads d_raw as one 16-B row per sample: raw and d_raw
 * must be 16-B aligned, or the call returns CN_EINVAL without a launch. */

/* Floats needed for one packed model of format fmt (cn_mlp_pack output); -1 for a bad fmt. */
int64_t cn_mlp_packed_floats(int fmt);

/* Pack a CodeNeRFModel state_dict (model.py:145-156) into the MFMA fragment
 * layout the field kernel streams.  params: HOST array of CN_NUM_PARAMS device
 * pointers in state_dict order (layer_xyz1.weight, layer_xyz1.bias, layer_xyz2.*,
 * fc_out.*, shape_code_layer1.*, shape_code_layer2.*, texture_code_layer1.*,
 * layer_dir1.*, layer_dir2.*, fc_rgb.*). */
int cn_mlp_pack(const float* const* params, int fmt, float* packed, cn_stream_t stream);

/* The per-object terms of CodeNeRFModel.forward that the reference recomputes
 * for every sample (model.py:174-177 and the code halves of :180-192), once
 * per code row: out row i = [W_xyz2[:,256:] zs1 + b_xyz2 | W_out[:,256:] zs2 + b_out |
 * W_rgb[:,256:] zt1 + b_rgb | 0 0 0 0] with zs1/zs2/zt1 the relu'd code layers.
 * z_s, z_t: (n_codes, 256); code_bias: (n_codes, CN_CODE_BIAS_STRIDE). */
int cn_code_bias(const float* const* params, const float* z_s, const float* z_t,
                 int64_t n_codes, float* code_bias, cn_stream_t stream);

/* The per-code bias of the folded layer (CN_FMT_F32_W16_FOLD): fold_bias row i =
 * W_dir1[:, :256] c_feat[i] + b_dir1, c_feat the second 256 floats of code_bias row i (cn_code_bias),
 * accumulated in double and rounded once.  code_bias: (n_codes, CN_CODE_BIAS_STRIDE); fold_bias:
 * (n_codes, 256).  One small launch. */
int cn_fold_bias(const float* const* params, const float* code_bias, int64_t n_codes, float* fold_bias,
                 cn_stream_t stream);

/* Everything a step needs from a model's weights and codes before its fp32 field kernels, in ONE
 * launch (what the reference recomputes inside every CodeNeRFModel.forward, model.py:160-194):
 * code_bias as cn_code_bias (NULL: skipped), packed / packed_t as cn_mlp_pack with CN_FMT_F32_W16
 * / CN_FMT_F32_W16_T (each NULL: skipped), and zero[0 .. n_zero) set to 0 (the fused backward's
 * g_code accumulator).  Bitwise the outputs of the separate calls. */
int cn_field_prepare(const float* const* params, const float* z_s, const float* z_t, int64_t n_codes,
                     float* code_bias, float* packed, float* packed_t, float* zero, int64_t n_zero,
                     cn_stream_t stream);

/* One model's part of cn_field_prepare_models: the arguments of cn_field_prepare, and code_act
 * (optional, with code_bias; (n_codes, 768)): the code layers' activations s1 | s2 | t1 after the
 * ReLU (model.py:174-177) as this launch formed them, for cn_code_bias_backward_act. */
typedef struct cn_field_prep {
  const float* const* params;
  float* code_bias;
  float* packed;
  float* packed_t;
  float* zero;
  int64_t n_zero;
  float* code_act;
} cn_field_prep;

/* cn_field_prepare for n_models (1 or 2) models on the same codes in ONE launch: a render's coarse
 * and fine fields (nerf/__init__.py:74-91 runs both on one object's codes) prepared together before
 * the coarse field.  Bitwise each model's cn_field_prepare. */
int cn_field_prepare_models(const cn_field_prep* models, int n_models, const float* z_s, const float* z_t,
                            int64_t n_codes, cn_stream_t stream);

/* CodeNeRFModel.forward(z_s, z_t, x), model.py:160-194, for pre-encoded rows.
 * x: (m, 90) = [xyz 63 | dir 27]; code row of row i = code_index ? code_index[i]
 * : (n_codes == 1 ? 0 : i); raw: (m, 4) = [rgb_raw(3), sigma_raw]. */
int cn_mlp_forward(const float* packed, int fmt, const float* code_bias, const int64_t* code_index,
                   int64_t n_codes, const float* x, int64_t m, float* raw, cn_stream_t stream);

/* forward_pass, nerf/__init__.py:94-134: embed + MLP for a ray chunk list.
 * Points come from pts (n_rays, n_samples, 3) if non-NULL, else pts = ro + rd*z
 * with z: (n_rays, n_samples).  rays are cut into consecutive chunks of
 * chunk_rows (util.get_minibatches) and Q1 applies per chunk: sample row
 * k = r*S + s of a chunk of Rc rays takes the view direction of ray k mod Rc.
 * freqs_xyz (10) / freqs_dir (4): HOST arrays.  code row of ray r as in
 * cn_mlp_forward (with r for i).  raw: (n_rays, n_samples, 4). */
int cn_radiance_field(const float* packed, int fmt, const float* code_bias, const int64_t* code_index,
                      int64_t n_codes, const float* pts, const float* ro, const float* rd,
                      const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                      const float* freqs_xyz, const float* freqs_dir, float* raw,
                      cn_stream_t stream);

/* cn_mlp_forward / cn_radiance_field on a CN_FMT_F32_W16_FOLD pack: the same arguments plus
 * fold_bias (n_codes, 256), cn_fold_bias of the same code_bias rows.  raw's sigma_raw is bit for bit
 * the unfolded CN_FMT_F32_W16 kernel's; rgb_raw differs from it by the rounding of W_f and c_v1
 * (and is exact wherever the unfolded kernel is, i.e. while every partial sum is an integer below
 * 2^24).  Any other fmt returns CN_EUNSUPPORTED, as cn_mlp_forward / cn_radiance_field do for
 * CN_FMT_F32_W16_FOLD, before any other check and without a launch. */
int cn_mlp_forward_fold(const float* packed, int fmt, const float* code_bias, const float* fold_bias,
                        const int64_t* code_index, int64_t n_codes, const float* x, int64_t m, float* raw,
                        cn_stream_t stream);
int cn_radiance_field_fold(const float* packed, int fmt, const float* code_bias, const float* fold_bias,
                           const int64_t* code_index, int64_t n_codes, const float* pts, const float* ro,
                           const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                           int64_t chunk_rows, const float* freqs_xyz, const float* freqs_dir, float* raw,
                           cn_stream_t stream);

/* Per-ray view-direction rows for cn_radiance_field_fold_rows.  Under Q1 (nerf/__init__.py:127-128) a
 * sample takes the view direction of ray k mod Rc of its chunk, so a launch of n_rays rays holds only
 * n_rays distinct directions, each used n_samples times; layer_dir1's view-direction term
 * (model.py:188-189) is therefore per-ray work.  Row r (256 floats, feature order) =
 * fold_bias row 0 + W_dir1[:, 256:] enc(rd[r] / |rd[r]|): bit for bit what cn_radiance_field_fold's
 * kernel holds after its view-direction chunk (the same normalisation, sin / cos evaluator and
 * matrix instructions in the same order).
 * cn_view_rows_bytes(n_rays): the table's size, 1 KiB per ray (256 MiB for 262,144 rays), or -1 for
 * n_rays <= 0 or a size past int64. */
int64_t cn_view_rows_bytes(int64_t n_rays);

/* Fill view_rows (cn_view_rows_bytes(n_rays) bytes, 16-byte aligned; every row written, nothing past
 * them) from packed (the CN_FMT_F32_W16_FOLD pack), fold_bias (cn_fold_bias; row 0 is read) and the
 * rays' directions rd (n_rays, 3).  freqs_dir (4): a HOST array.  One launch, 16 rays per wave.
 * CN_EUNSUPPORTED for another valid fmt; CN_EINVAL, before any launch: a NULL pointer, n_rays <= 0,
 * a misaligned packed / fold_bias / view_rows. */
int cn_view_rows(const float* packed, int fmt, const float* fold_bias, const float* rd, int64_t n_rays,
                 const float* freqs_dir, float* view_rows, cn_stream_t stream);

/* cn_radiance_field_fold with the view-direction term read from view_rows (cn_view_rows of the same
 * packed, fold_bias, rd, n_rays and freqs_dir) instead of computed per sample: the kernel neither
 * normalises a direction nor encodes it, and streams 27 weight chunks per tile instead of 28.  raw is
 * bit for bit cn_radiance_field_fold's for finite directions and frequencies inside the fast sin / cos
 * range (|f| max|d| <= 16384); beyond them the two agree in which outputs are NaN.  One code row only:
 * n_codes == 1 and code_index == NULL, anything else is CN_EINVAL.  A row costs one 1 KiB store and
 * n_samples 1 KiB loads: on MI355X the table is even at 4 samples per ray and pays from 8 on; for
 * single-sample lists use cn_radiance_field_fold. */
int cn_radiance_field_fold_rows(const float* packed, int fmt, const float* code_bias, const float* fold_bias,
                                const float* view_rows, const int64_t* code_index, int64_t n_codes,
                                const float* pts, const float* ro, const float* rd, const float* z,
                                int64_t n_rays, int64_t n_samples, int64_t chunk_rows, const float* freqs_xyz,
                                const float* freqs_dir, float* raw, cn_stream_t stream);

/* Density alone: sigma_raw of CodeNeRFModel.forward, model.py:174-186 (layer_xyz1, layer_xyz2 with
 * the shape code, fc_out row 0) -- the first 10 of the field kernel's 36 weight chunks, 163,840 of
 * its 572,416 FLOP per sample, and bit for bit the sigma_raw cn_radiance_field writes for the same
 * point and code (finite view directions).  Neither a view direction nor the texture code enters:
 * code_bias may be formed with any z_t.  fmt: CN_FMT_F32_W16 only (the other formats return
 * CN_EUNSUPPORTED before any launch); packed is that format's cn_mlp_pack, unchanged.
 * Exactly one input mode, m = n_rays * n_samples samples:
 *   pts (m, 3);
 *   ro, rd (n_rays, 3) and z (n_rays, n_samples): pts = ro + rd*z as cn_radiance_field forms them;
 *   x: m pre-encoded rows, x_stride (>= 63) floats apart, of which the 63 xyz columns are read
 *      ((m, 63) and (m, 90) rows both fit).
 * code row of sample k = that of ray r = k / n_samples, as in cn_radiance_field: code_index[r], or
 * row 0 (n_codes == 1), or row r (n_codes == n_rays).  freqs_xyz (10): a HOST array.
 * Outputs, either or both: sigma (m); raw (m, 4) rows [0, 0, 0, sigma_raw], 16-byte aligned, which
 * cn_volume_render and cn_sample_pdf take as they take a field's (their weights read sigma only).
 * CN_EINVAL before any launch: packed, code_bias or freqs_xyz NULL; not exactly one mode (or a
 * partial ro / rd / z); both outputs NULL; raw misaligned; a size <= 0; x_stride < 63; n_codes
 * neither 1 nor n_rays without a code_index. */
int cn_density_field(const float* packed, int fmt, const float* code_bias, const int64_t* code_index,
                     int64_t n_codes, const float* pts, const float* ro, const float* rd, const float* z,
                     const float* x, int64_t x_stride, int64_t n_rays, int64_t n_samples,
                     const float* freqs_xyz, float* sigma, float* raw, cn_stream_t stream);

/* The density's gradient: grad_sigma (m, 4) rows [d sigma_raw / d x, d / d y, d / d z, sigma_raw] of
 * CodeNeRFModel.forward's density (model.py:174-186) at m = n_rays * n_samples points -- surface normals
 * are -gradient / |gradient|.  One launch: cn_density_field's 10 weight chunks with both ReLU masks kept
 * in registers, then the last 10 chunks of the fused backward (layer_xyz2^T, layer_xyz1^T and the
 * encoding's derivative) with d sigma_raw = 1; 327,680 FLOP per point.  Column 3 is bit for bit
 * cn_density_field's sigma_raw; columns 0..2 equal, value for value, the d_pts that
 * cn_radiance_field_masks + cn_field_backward_fused give for d_raw = (0, 0, 0, 1).
 * packed: the CN_FMT_F32_W16 cn_mlp_pack (fmt), packed_t: the CN_FMT_F32_W16_T one (fmt_t), of the same
 * parameters, both unchanged; a valid forward / transposed pair in other formats returns
 * CN_EUNSUPPORTED before any launch.  Exactly one input mode:
 *   pts (m, 3);
 *   ro, rd (n_rays, 3) and z (n_rays, n_samples): pts = ro + rd*z as cn_radiance_field forms them; the
 *     gradient is with respect to that point (nothing flows to ro, rd or z).
 * code row of sample k = that of ray r = k / n_samples, as in cn_density_field: code_index[r], or row 0
 * (n_codes == 1), or row r (n_codes == n_rays).  freqs_xyz (10): a HOST array.
 * grad_sigma: 16-byte aligned, every row written (a non-finite point gives NaN).  Stream-ordered on
 * `stream`, no workspace, no synchronisation, nothing retained after return: capturable in a graph.
 * CN_EINVAL before any launch: a NULL packed, packed_t, code_bias, freqs_xyz or grad_sigma; not exactly
 * one mode (or a partial ro / rd / z); grad_sigma misaligned; a size <= 0; n_codes neither 1 nor n_rays
 * without a code_index; fmt not a forward format or fmt_t not a transposed one (unknown values, or the
 * two packs swapped). */
int cn_density_gradient(const float* packed, const float* packed_t, int fmt, int fmt_t, const float* code_bias,
                        const int64_t* code_index, int64_t n_codes, const float* pts, const float* ro,
                        const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                        const float* freqs_xyz, float* grad_sigma, cn_stream_t stream);

/* --- Occupancy-grid sample culling (inference) --------------------------
 * A grid is the cube [-bound, bound]^3 cut into g^3 cells, g a multiple of 32 in [32, 512], one bit
 * per cell in g^3 / 32 32-bit words of device memory: cell (ix, iy, iz) has linear index
 * c = (ix g + iy) g + iz and is occupied iff bit c & 31 of word c >> 5 is set.
 * Point lookup, fp32 with every operation rounded: u_d = (p_d - lo) * inv_cell (the caller passes
 * lo = -bound and inv_cell = (float)(g / (2 bound))); the point is inside iff 0 <= u_d < g on all
 * three axes (a NaN coordinate fails), its cell is i_d = (int)floorf(u_d); a point outside the
 * cube is empty.  A culled sample has exactly zero density -- not the field's softplus tail.
 * All three entries are stream-ordered, launch on `stream` and never synchronise; argument errors
 * return CN_EINVAL before any launch. */

/* sigma_raw of a culled slot of cn_occupancy_expand's output: softplus(x - 1) as cn_volume_render
 * evaluates it is exactly 0 there, so the slot has alpha 0, weight 0 and leaves the transmittance
 * as it was. */
#define CN_EMPTY_SIGMA_RAW (-1.0e4f)

/* Grid from node densities: nodes (g+1)^3, axis order [ix, iy, iz], the density at
 * linspace(-bound, bound, g+1) per axis.  A cell is occupied iff one of the nodes
 * [i_d - dilate, i_d + 1 + dilate] per axis (clamped to the node grid) is > threshold or NaN:
 * dilate = 0 tests the cell's 8 corners, dilate 1 or 2 grows that occupancy by as many cells in
 * Chebyshev distance.  One launch; bits: g^3 / 32 words, all written.
 * CN_EINVAL: nodes or bits NULL; g not a multiple of 32 in [32, 512]; dilate outside 0..2. */
int cn_occupancy_build(const float* nodes, int64_t g, float threshold, int dilate, uint32_t* bits,
                       cn_stream_t stream);

/* Bytes of the state workspace of cn_occupancy_cull / cn_occupancy_expand for (n_rays, n_samples)
 * (the rays' kept-sample offsets and kept masks), or -1 for sizes those entries refuse. */
int64_t cn_occupancy_cull_workspace_bytes(int64_t n_rays, int64_t n_samples);

/* Look up every sample k = r n_samples + s at p = ro[r] + rd[r] * z[r][s] (formed as
 * cn_radiance_field forms it) and compact the occupied ones, in ascending k, into M' rows:
 *   count[0]        M' (device int64);
 *   sample_index[j] k (int32);
 *   pts[j]          p (3 floats);
 *   vdir[j]         the UNNORMALISED rd row of the sample's Q1 view-direction ray (chunk_rows as in
 *                   cn_radiance_field: base = (r / chunk_rows) chunk_rows, rcnt = min(chunk_rows,
 *                   n_rays - base), ray base + ((r - base) n_samples + s) % rcnt);
 *   code_out[j]     (int64, optional) code_index ? code_index[r] : r.
 * Every output holds n_rays * n_samples rows, of which the first M' are written.  The rows are a
 * points-mode input of cn_radiance_field, cn_radiance_field_fold and cn_density_field -- pts, rd =
 * vdir, n_rays = chunk_rows = M', n_samples = 1, code_index = code_out (or none with one code
 * row) -- which computes for each the bits the unculled field computes for sample k.
 * workspace: cn_occupancy_cull_workspace_bytes(n_rays, n_samples) bytes, 8-byte aligned; contents on
 * entry are ignored; written here and read by cn_occupancy_expand.  Three launches (masks, a scan of
 * the rays' counts, emit): no atomics, the result is deterministic.
 * CN_EINVAL: a required pointer NULL (code_index and code_out are optional); n_rays <= 0;
 * n_samples outside 1..512; n_rays * n_samples > INT32_MAX; chunk_rows <= 0; g as above; workspace
 * or count not 8-byte aligned. */
int cn_occupancy_cull(const float* ro, const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                      int64_t chunk_rows, const int64_t* code_index, const uint32_t* bits, int64_t g,
                      float lo, float inv_cell, void* workspace, int64_t* count, int32_t* sample_index,
                      float* pts, float* vdir, int64_t* code_out, cn_stream_t stream);

/* The gather back: raw (n_rays, n_samples, 4) row k = raw_compact (M', 4) row j where
 * sample_index[j] = k, and [0, 0, 0, CN_EMPTY_SIGMA_RAW] for a culled k.  workspace: what
 * cn_occupancy_cull (or cn_weight_cull) of the same sizes left there, only read here.  raw and
 * raw_compact 16-byte aligned; raw_compact may be NULL only when the caller knows M' = 0.
 * CN_EINVAL: workspace or raw NULL; a size cn_occupancy_cull refuses; raw or raw_compact
 * misaligned; workspace not 8-byte aligned. */
int cn_occupancy_expand(const float* raw_compact, const void* workspace, int64_t n_rays, int64_t n_samples,
                        float* raw, cn_stream_t stream);

/* --- Per-ray depth spans (inference) -------------------------------------
 * Where the coarse samples go: each ray gets its own depth interval, from just before its first
 * occupied grid cell to just after its last, and its nc coarse depths are stratified uniformly inside
 * it.  Linear in depth only; the gaps inside a span are not skipped.  fp32, every operation rounded on
 * its own, no FMA.  For ray r, K objects (1 <= K <= CN_MAX_SCENE_OBJECTS) each with its own rays
 * ro_k, rd_k in its own frame (cn_object_rays: a rigid pose keeps the ray parameter) and its grid
 * (bits_k, g_k, lo_k, inv_cell_k), near < far, P = n_probes:
 *   probe depths  step = (far - near) / (float)(P - 1);  d_j = near + (float)j * step for j < P - 1,
 *                 d_{P-1} = far exactly;
 *   probe lookup  probe j is occupied iff for some k the point lookup above finds a set bit at
 *                 p = rd_k[r] * d_j + ro_k[r] (product and sum each rounded, as cn_occupancy_cull forms
 *                 it); a NaN or out-of-cube point is unoccupied;
 *   span indices  first / last = the lowest / highest occupied j.  None: the ray is a MISS, first =
 *                 last = -1, a = 0, b = P - 1 (it keeps the whole range; the grid culls its samples as
 *                 before).  Otherwise a = max(first - 1, 0), b = min(last + 1, P - 1); b > a always;
 *   depths        t_lo = d_a, t_hi = d_b, w = (t_hi - t_lo) / (float)(nc - 1);
 *                 z_i = min(t_lo + ((float)i + tau_i) * w, t_hi) for i <= nc - 2, tau_i = t_rand[r][i]
 *                 (0 without t_rand);  z_{nc-1} = t_hi exactly, always.
 * Every rounding is monotone, so a row is non-decreasing (ties can occur: tau may be the largest float
 * below 1).  volume_render gives the last sample the 1e10 interval; when last < P - 1, z_{nc-1} has the
 * bits of an unoccupied probe, cn_occupancy_cull forms the same point from them, and the sample is culled
 * for every object: the last real sample's interval ends at t_hi, not at infinity.  When last = P - 1
 * the ray ends inside occupied space at far, as the plain sampler's does.
 * The span is not strictly conservative: an occupied cell crossed only between two unoccupied probes
 * outside [a, b] (a corner clip shorter than one probe step) is left out; a grid dilated by one cell
 * (cn_occupancy_build's dilate = 1) covers that. */

/* The rule above.  ro, rd: device (n_objects, n_rays, 3).  bits (device pointers), g, lo, inv_cell: HOST
 * arrays of n_objects.  n_probes: a multiple of 64 in [64, 1024]; nc in [2, 512].  t_rand: (n_rays, nc)
 * -- cn_sample_uniform's shape, columns 0 .. nc - 2 are read -- or NULL.  Outputs, every element
 * written: z_out (n_rays, nc); span (n_rays, 2) = (t_lo, t_hi); probe_range (n_rays, 2) int32 =
 * (first, last).  One launch on `stream`: no workspace, no atomics, no synchronisation.
 * CN_EINVAL before any launch: a required pointer or an entry of bits NULL; n_objects outside
 * 1..CN_MAX_SCENE_OBJECTS; n_rays <= 0; n_probes or nc outside the ranges above; a g[k] that
 * cn_occupancy_build refuses; near or far not finite, near < 0 or far <= near; an inv_cell[k] or lo[k]
 * that is not finite. */
int cn_sample_span(const float* ro, const float* rd, int64_t n_rays, const uint32_t* const* bits,
                   const int64_t* g, const float* lo, const float* inv_cell, int n_objects, float near,
                   float far, int64_t n_probes, int64_t nc, const float* t_rand, float* z_out, float* span,
                   int32_t* probe_range, cn_stream_t stream);

/* --- Weight-bounded colour culling (inference) --------------------------
 * A ray's volume-render weights depend on its densities alone, so a pass that has the densities of
 * every sample (cn_density_field) and their weights (cn_volume_render) can leave out the colour
 * layers of the samples whose weight cannot matter.  For one ray with fp32 weights w[0..S-1]:
 *   tail_i = sum_{k >= i} (double)w_k, accumulated in double;
 *   sample i is KEPT iff w_i > 0, w_i >= eps_weight (an fp32 comparison) and tail_i >= (double)eps_tail.
 * A NaN fails every test: a NaN sample, and every sample before it (their tails are NaN), is culled.
 * Order of the double additions: the samples in words of 64 (word v = samples 64 v .. 64 v + 63,
 * missing ones 0), the last word first; in a word, lane l's sum is built in log steps (+ lane l + 1,
 * + the pair at l + 2, + the four at l + 4, ...), then the total of the later words is added.  For
 * weights that are multiples of 2^-30 (any sum of <= 512 of them below 2^23 is exact) every order
 * gives the same tails.
 * A caller with a tolerance tol on the composited colour passes eps_tail = tol / 2 and eps_weight =
 * the largest float <= tol / (2 S): the culled tail of a ray then sums to < tol / 2 and each of the
 * at most S other culled samples is < tol / (2 S), so the culled weights of a ray sum to <= tol.
 * A culled sample keeps its sigma_raw and takes raw colours [0, 0, 0], which composite as 0.5, while
 * a true colour lies in [-0.001, 1.001]: weights, depth, acc and disp keep the plain render's bits
 * and each colour channel moves by <= 0.501 * (the ray's culled weight) <= 0.501 tol, plus the fp32
 * rounding of the two S-term sums compared. */

/* cn_occupancy_cull with the kept test above in place of the grid lookup: weights (n_rays,
 * n_samples) as cn_volume_render wrote them.  Every output, the workspace
 * (cn_occupancy_cull_workspace_bytes; contents on entry are ignored) and its layout are
 * cn_occupancy_cull's -- the same scan and emit launches follow the mask launch -- so
 * cn_occupancy_expand reads the state it leaves.
 * Stream-ordered, no atomics, compact rows in ascending k.
 * CN_EINVAL before any launch: weights NULL; eps_weight or eps_tail negative or NaN; and every
 * size, pointer and alignment rule of cn_occupancy_cull. */
int cn_weight_cull(const float* weights, const float* ro, const float* rd, const float* z, int64_t n_rays,
                   int64_t n_samples, int64_t chunk_rows, const int64_t* code_index, float eps_weight,
                   double eps_tail, void* workspace, int64_t* count, int32_t* sample_index, float* pts,
                   float* vdir, int64_t* code_out, cn_stream_t stream);

/* Components 0..2 of raw (n_slots, 4) row sample_index[j] = those of raw_compact (n_rows, 4) row j,
 * for j < n_rows; component 3 (sigma_raw) and every row not indexed are left as they are, so what
 * cn_volume_render derives from the densities cannot change.  An index outside 0..n_slots - 1
 * writes nothing.  Rows must be indexed at most once (cn_weight_cull's are).  One launch.
 * CN_EINVAL: a pointer NULL; n_rows outside 1..n_slots; n_slots > INT32_MAX; raw_compact or raw not
 * 16-byte aligned. */
int cn_scatter_rgb(const float* raw_compact, const int32_t* sample_index, int64_t n_rows, float* raw,
                   int64_t n_slots, cn_stream_t stream);

/* --- Counted field calls: the row count in device memory (inference) ------
 * cn_occupancy_cull and cn_weight_cull leave M' in device memory, and the calls above over their compact
 * rows take it as a host integer: a caller must read it back, which synchronises the host and keeps the
 * render out of a captured graph.  The counted entries take the CAPACITY n_rows_max of the compact
 * buffers (n_rays * n_samples of the cull) and `count`, a device int64, 8-byte aligned -- the cull's.
 * The launch is sized by the capacity and the kernel reads count[0] when it runs, so a graph replay
 * follows the count of its own cull.  Let k = min(max(count[0], 0), n_rows_max):
 *   rows j < k of every output hold exactly the bits the uncounted entry computes for rows 0 .. k-1 with
 *     n_rays = chunk_rows = k (inside the kernel n_rays = chunk_rows = n_rows_max: with one sample per
 *     row the Q1 ray of row j is j for any chunk_rows >= n_rays, in the folded decode too);
 *   rows j >= k of every output are not written;
 *   rows j >= k of every input (pts, rd, code_index, sample_index, raw_compact) may hold anything, NaN
 *     and out-of-range code_index values included: they influence nothing, and no address is formed
 *     from them (a partial tile's idle lanes repeat row k - 1; with k = 0 no row is decoded at all).
 * Each is one launch on `stream`, without synchronisation or atomics; count[0] must not change between
 * the launch and its completion other than by work ordered before it on the stream.
 * The three field entries: fp32 16x16x4 kernels only -- cn_radiance_field_counted and
 * cn_density_field_counted take CN_FMT_F32_W16, cn_radiance_field_fold_counted CN_FMT_F32_W16_FOLD -- in
 * the points form: pts (n_rows_max, 3), n_samples = 1, for the radiance entries rd (n_rows_max, 3) the
 * rows' own view directions (cn_occupancy_cull's vdir); one code row (n_codes = 1) or code_index
 * (n_rows_max).  ro, z (and the density entry's rd) are in the signature as in the parents' and must
 * be NULL.  Every other argument is the parent's.
 * CN_EINVAL before any launch: count NULL or not 8-byte aligned; n_samples != 1; ro or z given; pts NULL;
 * n_rows_max <= 0; any other format; neither code_index nor n_codes = 1; and the parent's pointer and
 * alignment rules. */
int cn_radiance_field_counted(const float* packed, int fmt, const float* code_bias, const int64_t* code_index,
                              int64_t n_codes, const float* pts, const float* ro, const float* rd, const float* z,
                              int64_t n_rows_max, int64_t n_samples, const int64_t* count, const float* freqs_xyz,
                              const float* freqs_dir, float* raw, cn_stream_t stream);
int cn_radiance_field_fold_counted(const float* packed, int fmt, const float* code_bias, const float* fold_bias,
                                   const int64_t* code_index, int64_t n_codes, const float* pts, const float* ro,
                                   const float* rd, const float* z, int64_t n_rows_max, int64_t n_samples,
                                   const int64_t* count, const float* freqs_xyz, const float* freqs_dir, float* raw,
                                   cn_stream_t stream);
int cn_density_field_counted(const float* packed, int fmt, const float* code_bias, const int64_t* code_index,
                             int64_t n_codes, const float* pts, const float* ro, const float* rd, const float* z,
                             int64_t n_rows_max, int64_t n_samples, const int64_t* count, const float* freqs_xyz,
                             float* sigma, float* raw, cn_stream_t stream);

/* cn_scatter_rgb with n_rows = k of the rule above: raw_compact (n_rows_max, 4), sample_index
 * (n_rows_max); the indices in rows >= k are not read.  One launch over n_rows_max rows.
 * CN_EINVAL: a pointer NULL; count not 8-byte aligned; n_rows_max outside 1..n_slots; n_slots >
 * INT32_MAX; raw_compact or raw not 16-byte aligned. */
int cn_scatter_rgb_counted(const float* raw_compact, const int32_t* sample_index, const int64_t* count,
                           int64_t n_rows_max, float* raw, int64_t n_slots, cn_stream_t stream);

/* --- Scene composition (inference) --------------------------------------
 * Several posed objects in one image.  A rigid pose keeps the ray parameter -- the world point
 * ro + z rd is ro' + z rd' in the object's frame (cn_object_rays) -- so every object is sampled at the
 * same depths z[r][s] along the world ray, and the K objects' raw rows of a sample become one ray
 * integral by the rule below (cn_volume_render_compose).  Every implementation follows it.
 * For sample (r, s) and objects k = 0 .. K-1 with raw rows raw_k[r][s] = (x0, x1, x2, xs):
 *   sigma_k = softplus20(xs - 1) and c_k[ch] = sigmoid(x_ch) * 1.002 - 0.001, cn_volume_render's
 *     expressions with its intrinsics;
 *   sigma = ((0 + sigma_0) + sigma_1) + ..., fp32, ascending k;
 *   object k is ACTIVE at the sample iff sigma_k != 0 (a NaN density is active);
 *   colour c, by the number of active objects: none (0, 0, 0); exactly one (object a) c_a as it is;
 *     two or more c[ch] = (sum_k sigma_k c_k[ch]) / sigma over the active k, ascending, from 0, every
 *     product, sum and the division rounded in fp32 (an inactive object's row contributes nothing,
 *     whatever its colours hold);
 *   share_k: 0 for an inactive object, 1 for the only active one, else sigma_k / sigma (fp32).
 * sigma and c then go through cn_volume_render's arithmetic unchanged: dist with the 1e10 last
 * interval, delta = dist |rd|, the double-precision exclusive scan of sigma delta, trans, alpha and w,
 * the per-lane runs and the order in which rgb, depth and acc are summed, disp, and the sample-free
 * n_samples = 1 case.  acc_objects[k][r] = sum_s w_s share_k,s, summed in acc's order, is object k's
 * instance mask.
 * Consequences: a slot culled by cn_occupancy_expand (CN_EMPTY_SIGMA_RAW) is inactive; a ray whose
 * every sample has at most one active object gets, bit for bit, what cn_volume_render returns for the
 * raw tensor holding each sample's active row, whatever the order of the objects; one object is
 * cn_volume_render. */
#define CN_MAX_SCENE_OBJECTS 8

/* The rule above.  raws: HOST array of n_objects device pointers to (n_rays, n_samples, 4) tensors;
 * z, rd and the outputs as in cn_volume_render; weights (n_rays, n_samples) and acc_objects
 * (n_objects, n_rays) may be NULL.  Every raws[k], z and weights 16-B aligned.  One launch on
 * `stream`: no workspace, no atomics, no synchronisation.
 * CN_EINVAL before any launch: a required pointer or an entry of raws NULL; n_objects outside
 * 1..CN_MAX_SCENE_OBJECTS; n_rays <= 0; n_samples outside 1..512; a misaligned tensor. */
int cn_volume_render_compose(const float* const* raws, int n_objects, const float* z, const float* rd,
                             int64_t n_rays, int64_t n_samples, float* rgb, float* disp, float* acc,
                             float* weights, float* depth, float* acc_objects, cn_stream_t stream);

/* World rays (n_rays, 3) in the frame of each of n_objects posed objects -> ro_out, rd_out
 * (n_objects, n_rays, 3), one launch.  poses: HOST array of n_objects x 12 floats, the object-to-world
 * rotation R row-major, then the translation t.  fp32, every operation rounded, no FMA:
 *   d = ro - t;  ro_out[i] = (d_0 R_0i + d_1 R_1i) + d_2 R_2i;  rd_out[i] the same with rd for d.
 * The identity pose returns the input's values (a -0.0 component may come back as +0.0).  The outputs
 * must not overlap the inputs.
 * CN_EINVAL: a pointer NULL; n_rays <= 0; n_objects outside 1..CN_MAX_SCENE_OBJECTS; a pose entry
 * that is not finite. */
int cn_object_rays(const float* ro, const float* rd, int64_t n_rays, const float* poses, int n_objects,
                   float* ro_out, float* rd_out, cn_stream_t stream);

/* --- Scene composition with uniform scale: similarity poses --------------
 * A similarity pose is 13 floats: R row-major (object to world), t, and the scale s, finite and > 0: how many
 * times larger than its canonical size the object appears.  A medium enlarged by s has extinction
 * sigma(x / s) / s, so the opacity along a chord through the object does not depend on its size; and dividing
 * the object-frame ray by s keeps the ray parameter, so one set of depths still serves every object.
 *   Object rays: u = cn_object_rays' result for (R, t), then ro_out[i] = u[i] / s, an IEEE division, rounded;
 *     rd_out the same from rd.  ro_out + z rd_out is the world point ro + z rd in the object's canonical frame.
 *   Composition: sigma_k = softplus20(xs - 1) / s_k, the division rounded in fp32; everything after that is the
 *     rule above on these sigma_k (active iff sigma_k != 0, the ascending sum, the three-case colour and share,
 *     cn_volume_render's integral with the world rd).  A culled slot stays exactly inactive (0 / s = 0).
 * With every s = 1 the scaled entries return the unscaled entries' bits.  The field kernels, the culls and the
 * samplers see object-frame rays and raw rows only, and are unchanged. */

/* cn_object_rays with HOST poses of n_objects x 13 floats (R, t, s).  One launch, no workspace.
 * CN_EINVAL: what cn_object_rays refuses; a scale that is NaN, infinite or <= 0. */
int cn_object_rays_scaled(const float* ro, const float* rd, int64_t n_rays, const float* poses, int n_objects,
                          float* ro_out, float* rd_out, cn_stream_t stream);

/* cn_volume_render_compose with the objects' scales: a HOST array scales[n_objects].  One launch, no workspace.
 * CN_EINVAL: what cn_volume_render_compose refuses; scales NULL; a scale that is NaN, infinite or <= 0. */
int cn_volume_render_compose_scaled(const float* const* raws, const float* scales, int n_objects, const float* z,
                                    const float* rd, int64_t n_rays, int64_t n_samples, float* rgb, float* disp,
                                    float* acc, float* weights, float* depth, float* acc_objects,
                                    cn_stream_t stream);

/* --- Iso-surface extraction (inference) ---------------------------------
 * A node grid to a triangle mesh, on the device: marching tetrahedra on the Kuhn (Freudenthal) split
 * of each cell.  The split is the same in every cell, so neighbouring cells agree on every shared
 * face diagonal and the surface is closed wherever it does not leave the grid; there are no
 * ambiguous cases.
 * Input: nodes (n, n, n) fp32, axis order [ix, iy, iz], node a = (ix, iy, iz) at linear index
 * (ix n + iy) n + iz (what density_grid leaves); axis: n fp32 node coordinates, used on all three
 * axes; iso: the level, finite; 2 <= n <= 513.
 * Inside: a node is inside iff nodes[a] > iso -- a NaN and a value equal to iso are outside.
 * Corners and edges: cube corner k in 0..7 of the cell with lower node p is p + off(k), off(k) =
 * ((k >> 2) & 1, (k >> 1) & 1, k & 1) (x the most significant bit).  Every edge of the split runs
 * from a node a to a + off(k), k in 1..7: direction d = k - 1, owned by its lower node a.  Edge (a, d)
 * exists iff a + off(d + 1) is a node, and is active iff it exists and exactly one end is inside.
 * Vertices: one per active edge; its id is the rank of the key a * 7 + d (a linear) among the active
 * edges, ascending.  With b the upper node, t = (iso - v_a) / (v_b - v_a) and, per component c,
 * pos_c = axis[a_c] + t * (axis[b_c] - axis[a_c]): fp32, every operation rounded on its own, a true
 * division.  t is in [0, 1] for finite values; an infinite or NaN value gives what IEEE arithmetic
 * gives (a NaN t makes all three components NaN; which NaN -- sign, payload -- is not specified).
 * Tetrahedra: cell c = (ix (n - 1) + iy) (n - 1) + iz has six, tau = 0..5 the tau-th permutation
 * (a, b, c) of the axes (x, y, z) in lexicographic order, with corners (in tetrahedron order)
 * 0, bit(a), bit(a) | bit(b), 7, where bit(x) = 4, bit(y) = 2, bit(z) = 1.
 * Triangles of a tetrahedron, as triples of its edges: none with 0 or 4 corners inside; with one
 * corner L alone on its side (1 or 3 inside) and the others P < Q < R in tetrahedron order,
 * (LP, LQ, LR); with A < B inside and C < D outside, (AC, AD, BD) then (AC, BD, BC).
 * Orientation: with each vertex at its edge's midpoint in index space, the normal (v1 - v0) x
 * (v2 - v0) must point from the centroid of the tetrahedron's inside corners to that of its outside
 * corners; if not, the last two entries are swapped.  Then the face is rotated cyclically so that its
 * smallest vertex id comes first.  Normals point out of the solid, towards the lower values.
 * Faces: int32 triples of vertex ids in ascending (c, tau, triangle) order.  A face of zero area is
 * possible (a node equal to iso gives t = 0 on its edges); the mesh stays combinatorially closed.
 * No atomics, no workgroup waits on another: the result is a pure function of the inputs.  Both
 * launching entries are stream-ordered and never synchronise; argument errors return CN_EINVAL
 * before any launch.  Not provided: vertex normals, simplification, vertex colours. */

/* Bytes of the workspace cn_isosurface_count fills and cn_isosurface_emit reads, or -1 for n outside
 * 2..513.  Layout, each array padded to a multiple of 16 bytes, N = n^3 nodes and B = ceil(N / 256)
 * workgroups: the nodes' words (uint32: bits 0..6 the mask of the active edges the node owns, bits
 * 7..10 its cell's triangle count, bits 11..18 the cell's inside bits by corner), their exclusive
 * vertex offsets (int32), their exclusive face offsets (int32), the workgroups' exclusive vertex
 * offsets (int32, B), their exclusive face offsets (int32, B):
 *   bytes = 3 * pad16(4 N) + 2 * pad16(4 B). */
int64_t cn_isosurface_workspace_bytes(int64_t n);

/* Classify every node, scan, and leave every node's vertex and face offsets in the workspace (three
 * launches): counts[0] = V, the number of vertices, counts[1] = T, the number of faces (device
 * int64).  workspace: cn_isosurface_workspace_bytes(n) bytes, 8-byte aligned; contents on entry are
 * ignored.
 * CN_EINVAL: nodes, workspace or counts NULL; n outside 2..513; iso NaN or infinite; workspace or
 * counts not 8-byte aligned. */
int cn_isosurface_count(const float* nodes, int64_t n, float iso, void* workspace, int64_t* counts,
                        cn_stream_t stream);

/* The mesh of the grid cn_isosurface_count classified (same nodes, n and iso; workspace as it left
 * it, only read here): vertices (max_vertices, 3) fp32 and faces (max_faces, 3) int32.  A vertex or
 * face whose rank is >= its capacity is not stored and nothing is written past the capacity's rows;
 * a capacity of 0 skips that output, whose pointer may then be NULL.  One launch per output.
 * CN_EINVAL: nodes, axis or workspace NULL; n outside 2..513; iso NaN or infinite; a negative
 * capacity; a NULL output with a capacity above 0; workspace not 8-byte aligned. */
int cn_isosurface_emit(const float* nodes, const float* axis, int64_t n, float iso, const void* workspace,
                       int64_t max_vertices, int64_t max_faces, float* vertices, int32_t* faces,
                       cn_stream_t stream);

/* --- Iso-surface ray casting (inference) ---------------------------------
 * Where a ray first meets the level set sigma_raw = level: a search over S ascending depths per ray, then a
 * bisection of the bracketing pair, then one interpolation.  The densities come from the density entries
 * (cn_density_field, cn_density_gradient's column 3, cn_occupancy_expand's rows); the three entries here are
 * the per-ray search around them.  fp32, every operation named below rounded on its own, no FMA.
 * A value s is KNOWN iff s > CN_EMPTY_SIGMA_RAW: false for a culled slot's marker and for NaN.
 * A strided density: element i at ptr[i * stride], stride 1 (a plain array) or 4 (column 3 of (.., 4) raw
 * rows, the pointer passed already offset to that column).
 *   bracket  j = the smallest s in 0..S-1 with sigma[r][s] >= level (NaN compares false; a tie counts as
 *            reached).  No such j: hit = 0, lo = hi = S - 1.  j = 0 (the ray starts at or above the level):
 *            hit = 2, lo = hi = 0.  Otherwise hit = 1, lo = j - 1, hi = j.
 *            bracket[r] = [t_lo, t_hi, s_lo, s_hi] = [z[r][lo], z[r][hi], sigma[r][lo], sigma[r][hi]].
 *   step     update (only with a probe, only where hit = 1), sp = probe[r], the density at the previous t[r]:
 *            sp >= level ? (t_hi, s_hi) = (t, sp) : (t_lo, s_lo) = (t, sp) -- a NaN goes to the low end;
 *            next depth (finish = 0):  t = t_lo + 0.5f * (t_hi - t_lo);
 *            final depth (finish = 1): t = t_lo + w * (t_hi - t_lo), w = 1 when s_lo is not known or
 *            s_hi - s_lo <= 0, else w = min(max((level - s_lo) / (s_hi - s_lo), 0), 1): a true division, and
 *            a NaN quotient becomes 0 (the max and the min return their other operand);
 *            hit != 1 has t_lo = t_hi, both forms give that depth;
 *            point: pts[r][c] = ro[r][c] + rd[r][c] * t, the product and the sum each rounded (cn_ray_points).
 *   shade    hit != 0: rgb[r][c] = sigmoid(raw[r][c]) * 1.002 - 0.001, the expression cn_volume_render
 *            composites (the same device function); depth[r] = t[r]; pts[r] is left as it is.
 *            hit = 0: rgb[r] = background, depth[r] = +inf, pts[r] = NaN.
 * All three are one launch on `stream` over exactly n_rays rows: no workspace, no atomics, no count read
 * back, no synchronisation; argument errors return CN_EINVAL before any launch. */

/* The bracket rule.  sigma: strided, element (r, s) at sigma[(r n_samples + s) sigma_stride]; z (n_rays,
 * n_samples) ascending per ray.  Outputs, every element written: bracket (n_rays, 4), hit (n_rays) int32.
 * CN_EINVAL: a NULL pointer; n_rays <= 0; n_samples outside 2..1024; level NaN or infinite; sigma_stride
 * neither 1 nor 4. */
int cn_surface_bracket(const float* sigma, int64_t sigma_stride, const float* z, int64_t n_rays, int64_t n_samples,
                       float level, float* bracket, int32_t* hit, cn_stream_t stream);

/* The step rule.  ro, rd (n_rays, 3); hit (n_rays) int32; probe_sigma: strided (n_rays) or NULL (the first
 * call: no update, t is only written).  bracket (n_rays, 4), 16-byte aligned, and t (n_rays): read and
 * written in place; pts (n_rays, 3): every element written.
 * CN_EINVAL: ro, rd, hit, bracket, t or pts NULL; n_rays <= 0; level NaN or infinite; finish neither 0 nor 1;
 * probe_stride neither 1 nor 4; bracket misaligned. */
int cn_surface_step(const float* ro, const float* rd, const int32_t* hit, const float* probe_sigma,
                    int64_t probe_stride, float level, int finish, int64_t n_rays, float* bracket, float* t,
                    float* pts, cn_stream_t stream);

/* The shade rule.  raw (n_rays, 4), 16-byte aligned: the field's rows at the final points; hit, t (n_rays);
 * background: three HOST floats.  rgb (n_rays, 3) and depth (n_rays): every element written; pts (n_rays, 3):
 * only the rows of rays with hit = 0 are written.
 * CN_EINVAL: a NULL pointer; n_rays <= 0; raw misaligned. */
int cn_surface_shade(const float* raw, const int32_t* hit, const float* t, const float* background,
                     int64_t n_rays, float* rgb, float* depth, float* pts, cn_stream_t stream);

/* --- Backward (autograd through the eval / train step) ------------------
 * The gradients loss.backward() takes through the path in the reference's
 * test-time optimisation (view_synthesis/eval.py) and training step:
 * pose -> get_bundle -> sample -> sample_uniform / sample_pdf (depths
 * detached, point_sampler.py:115) -> forward_pass -> CodeNeRFModel.forward
 * -> volume_render.  All fp32. */

/* cn_radiance_field in fp32 that also stores the post-activation hidden rows
 * the backward needs: save = (5, M, 256) planes h1, h2, feat, v1, v2 with
 * M = n_rays * n_samples (layer_xyz1, layer_xyz2, fc_out[1:], layer_dir1,
 * layer_dir2 of model.py:179-191).  packed must be an fp32 (CN_FMT_F32) pack. */
int cn_radiance_field_train(const float* packed, const float* code_bias, const int64_t* code_index,
                            int64_t n_codes, const float* pts, const float* ro, const float* rd,
                            const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                            const float* freqs_xyz, const float* freqs_dir, float* raw, float* save,
                            cn_stream_t stream);

/* cn_mlp_forward in fp32 that also stores the (5, m, 256) activations (as above). */
int cn_mlp_forward_train(const float* packed, const float* code_bias, const int64_t* code_index,
                         int64_t n_codes, const float* x, int64_t m, float* raw, float* save,
                         cn_stream_t stream);

/* The (M, 90) rows forward_pass hands CodeNeRFModel.forward (nerf/__init__.py:116-132):
 * [posenc(pts) 63 | posenc(Q1 view dir) 27].  pts, or ro + z. */
int cn_encode_inputs(const float* pts, const float* ro, const float* rd, const float* z, int64_t n_rays,
                     int64_t n_samples, int64_t chunk_rows, const float* freqs_xyz, const float* freqs_dir,
                     float* x, cn_stream_t stream);

/* Floats of scratch cn_field_backward needs for M sample rows (workspace: contents on entry are
 * ignored). */
int64_t cn_field_backward_workspace_floats(int64_t m);
/* Offset (floats) of the (M, 90) dL/dx rows inside that scratch after cn_field_backward. */
int64_t cn_field_backward_dx_offset(int64_t m);

/* Backward of forward_pass + CodeNeRFModel.forward (model.py:160-194) from
 * d_raw (M, 4).  saved / x_enc from cn_radiance_field_train / cn_encode_inputs.
 * grads: 18 pointers (model.py parameter order, same as params) ACCUMULATED
 * into (+=), or NULL for no parameter gradients; the code-layer parameters
 * (shape/texture_code_layer*) and the code halves of layer_xyz2 / fc_out /
 * fc_rgb get their gradients from cn_code_bias_backward instead.
 * g_code: (n_codes, CN_CODE_BIAS_STRIDE) accumulated gradient of the
 * per-object code terms (cn_code_bias layout), or NULL.
 * d_pts (M, 3) is written when the inputs were pts; d_ro / d_rd (n_rays, 3) are
 * ACCUMULATED into (view-direction and, for ro + z inputs, point gradients).
 * With d_pts, d_ro and d_rd all NULL, pts / ro / rd / z / freqs may be NULL too
 * (rows from cn_mlp_forward_train: n_rays = M, n_samples = 1).  On return
 * workspace[2*260*M, 2*260*M + 90*M) holds dL/dx_enc (M, 90). */
int cn_field_backward(const float* const* params, const float* saved, const float* x_enc,
                      const float* d_raw, const float* pts, const float* ro, const float* rd,
                      const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                      const int64_t* code_index, int64_t n_codes, const float* freqs_xyz,
                      const float* freqs_dir, float* workspace, float* const* grads, float* g_code,
                      float* d_pts, float* d_ro, float* d_rd, cn_stream_t stream);

/* cn_field_backward with the GEMMs' arithmetic chosen by fmt: CN_FMT_F32 (exact-product
 * fp32 MFMA, what cn_field_backward runs) or CN_FMT_BF16X3 (every dX / dW GEMM as
 * Ah.Bh + Ah.Bl + Al.Bh on bf16 MFMA with fp32 accumulation, ~2^-17 relative error per
 * product; the training step).  Same arguments, outputs and workspace (contents on entry are ignored)
 * otherwise. */
int cn_field_backward_fmt(int fmt, const float* const* params, const float* saved, const float* x_enc,
                          const float* d_raw, const float* pts, const float* ro, const float* rd,
                          const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                          const int64_t* code_index, int64_t n_codes, const float* freqs_xyz,
                          const float* freqs_dir, float* workspace, float* const* grads, float* g_code,
                          float* d_pts, float* d_ro, float* d_rd, cn_stream_t stream);

/* --- Fused 3xbf16 backward (eval-step gradients, frozen weights) ---------
 * The gradients eval.py's loss.backward() takes into the codes and the pose
 * (eval.py:141-160; the reference's weight gradients are never read there).
 * Forward: cn_radiance_field_masks = cn_radiance_field on a CN_FMT_BF16X3 pack
 * that also writes the ReLU masks of layer_xyz1 / layer_xyz2 / layer_dir1 /
 * layer_dir2 (cn_field_mask_words(M) uint32 words; the bits of the last 128-sample tile's rows
 * past M are whatever the kernel leaves and no backward reads them).  Backward: one launch from
 * d_raw (M, 4) through the whole field on a CN_FMT_BF16X3_T pack of the same
 * weights: g_code (n_codes, CN_CODE_BIAS_STRIDE) ACCUMULATED as in
 * cn_field_backward (feed cn_code_bias_backward for dz_s / dz_t), d_pts (M, 3)
 * written for pts inputs, d_ro / d_rd (n_rays, 3) ACCUMULATED.  Needs one code
 * row per 32 consecutive samples (n_codes == 1, or n_samples % 32 == 0), else
 * CN_EUNSUPPORTED (use cn_field_backward). */
int64_t cn_field_mask_words(int64_t m);
int cn_radiance_field_masks(const float* packed, const float* code_bias, const int64_t* code_index,
                            int64_t n_codes, const float* pts, const float* ro, const float* rd,
                            const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                            const float* freqs_xyz, const float* freqs_dir, float* raw, uint32_t* masks,
                            cn_stream_t stream);
int cn_field_backward_x3(const float* packed_t, const uint32_t* masks, const float* d_raw, const float* pts,
                         const float* ro, const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                         int64_t chunk_rows, const int64_t* code_index, int64_t n_codes,
                         const float* freqs_xyz, const float* freqs_dir, float* g_code, float* d_pts,
                         float* d_ro, float* d_rd, cn_stream_t stream);

/* The same pair in either arithmetic.  fmt CN_FMT_BF16X3 (as above) or CN_FMT_F32_W16: the
 * fp32 16x16x4 inference kernel (exact fp32 products, the reference's arithmetic) that also
 * writes its ReLU masks (cn_field_mask_words_fmt(fmt, M) words).  The backward takes the
 * matching transposed pack (fmt_t CN_FMT_BF16X3_T / CN_FMT_F32_W16_T) and needs one code row
 * per wave: n_codes == 1, or n_samples % 32 (bf16x3) / % 16 (fp32) == 0. */
int64_t cn_field_mask_words_fmt(int fmt, int64_t m);
int cn_radiance_field_masks_fmt(int fmt, const float* packed, const float* code_bias, const int64_t* code_index,
                                int64_t n_codes, const float* pts, const float* ro, const float* rd,
                                const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                const float* freqs_xyz, const float* freqs_dir, float* raw, uint32_t* masks,
                                cn_stream_t stream);
int cn_field_backward_fused(int fmt_t, const float* packed_t, const uint32_t* masks, const float* d_raw,
                            const float* pts, const float* ro, const float* rd, const float* z, int64_t n_rays,
                            int64_t n_samples, int64_t chunk_rows, const int64_t* code_index, int64_t n_codes,
                            const float* freqs_xyz, const float* freqs_dir, float* g_code, float* d_pts,
                            float* d_ro, float* d_rd, cn_stream_t stream);
/* The same backward without float atomics (eval.py:145-160's backward, bit-reproducible): with
 * n_codes == 1 and, for bf16x3, n_samples % 32 == 0 the kernel writes per-workgroup g_code
 * rows and per-wave / per-sample ray-gradient terms (fp32 with n_samples % 16 != 0: the points' terms per
 * sample too, 6 floats each instead of 6 per wave of 16) into workspace
 * (cn_field_backward_fused_workspace_floats(fmt_t, n_rays, n_samples) floats, 16-B aligned; contents on
 * entry are ignored: a wave or workgroup without rows stores its zero row or is skipped by the sums),
 * and two short launches add them into g_code, d_ro and d_rd in a fixed order (g_code / d_ro / d_rd are
 * still ACCUMULATED).  Other shapes, or workspace NULL, run cn_field_backward_fused. */
int64_t cn_field_backward_fused_workspace_floats(int fmt_t, int64_t n_rays, int64_t n_samples);
int cn_field_backward_fused_ws(int fmt_t, const float* packed_t, const uint32_t* masks, const float* d_raw,
                               const float* pts, const float* ro, const float* rd, const float* z, int64_t n_rays,
                               int64_t n_samples, int64_t chunk_rows, const int64_t* code_index, int64_t n_codes,
                               const float* freqs_xyz, const float* freqs_dir, float* g_code, float* d_pts,
                               float* d_ro, float* d_rd, float* workspace, cn_stream_t stream);
/* The eval step's two fields (eval.py:153-167: predict_radiance_and_render's coarse and fine fields on the
 * same rays; the fine depths are detached, point_sampler.py:115, so the two backwards are independent) in
 * shared launches: each field the arguments of one cn_field_backward_fused_ws call, both adding into the
 * same d_ro / d_rd.  fp32, rays + depths, one code row, whole waves per ray: one dX launch and one ray /
 * g_code launch for both; d_ro / d_rd and g_code bitwise those of field 0's call,
 * then d_rd += d_rd_between (optional, n_rays x 3: the rays' gradient that arrives between the two
 * backwards -- the coarse volume render's), then field 1's call -- which is how fields that cannot share
 * run.  n_fields 1 or 2 (d_rd_between: 2 only). */
typedef struct cn_field_fused_bwd {
  const float* packed_t;
  const uint32_t* masks;
  const float* d_raw;
  const float* pts;
  const float* ro;
  const float* rd;
  const float* z;
  int64_t n_rays, n_samples, chunk_rows;
  const int64_t* code_index;
  int64_t n_codes;
  const float* freqs_xyz;
  const float* freqs_dir;
  float* g_code;
  float* d_pts;
  float* d_ro;
  float* d_rd;
  float* workspace;
} cn_field_fused_bwd;
int cn_field_backward_fused_multi(int fmt_t, const cn_field_fused_bwd* fields, int n_fields, const float* d_rd_between,
                                  cn_stream_t stream);

/* --- Fused fp32 training step (train.py:92-114; weights trained) ------------------
 * Forward: cn_radiance_field on a CN_FMT_F32_W16 pack that also writes the ReLU masks
 * (cn_field_mask_words_fmt(CN_FMT_F32_W16, M) words), the (5, M, 256) post-activation planes
 * h1, h2, feat, v1, v2 (cn_radiance_field_train's layout) and after them, at save + 5 M 256, the
 * (M, 64) encoding plane: the positional encodings layer_xyz1 multiplied, 16 per lane group in the
 * kernel's k-step order (column c' -> PositionalEmbedder column of the mlp_common.h map, one padding
 * slot).  save holds cn_field_train_saved_floats(CN_FMT_F32_W16, M) floats.
 * Backward: the fused dX chain of cn_field_backward_fused on the CN_FMT_F32_W16_T pack (g_code,
 * d_pts / d_ro / d_rd as there; g_code required) that also writes every layer's masked input
 * gradient into workspace (cn_field_backward_train_workspace_floats(M) floats; contents on entry are
 * ignored, the partial tiles of the dW plans included), then the weight
 * and bias gradients dW = dPre^T X as split-M fp32 MFMA GEMMs over those planes, saved and x_enc
 * (cn_encode_inputs; or x_enc NULL: the forward's own encodings from saved's encoding plane, fp32,
 * or generated inside the dW kernels, bf16x3), reduced
 * deterministically (cn_gemm_tn_ws) through the rest of workspace: grads (18 pointers, or NULL for none) ACCUMULATED as in
 * cn_field_backward (the code-layer parameters and code halves come from cn_code_bias_backward).
 * One code row per 16-sample wave: n_codes == 1 or n_samples % 16 == 0, else CN_EUNSUPPORTED. */
int cn_radiance_field_train_w16(const float* packed, const float* code_bias, const int64_t* code_index,
                                int64_t n_codes, const float* pts, const float* ro, const float* rd,
                                const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                const float* freqs_xyz, const float* freqs_dir, float* raw, float* save,
                                uint32_t* masks, cn_stream_t stream);
/* The same pair for either precision: fmt CN_FMT_F32_W16 (fp32 16x16x4) or CN_FMT_BF16X3 (3xbf16
 * 32x32x16; masks cn_field_mask_words_fmt(CN_FMT_BF16X3, M) words, the same fp32 planes), and
 * fmt_t the matching transposed pack (CN_FMT_F32_W16_T / CN_FMT_BF16X3_T; the bf16x3 dW GEMMs
 * are 3xbf16 too).  bf16x3: one code row per 32-sample wave (n_codes == 1 or n_samples % 32 == 0);
 * its save buffer holds 5 * M * 256 + 256 floats (the last row is scratch for padding lanes: contents
 * on entry are ignored, and what it holds afterwards is unspecified and never read).
 * cn_field_train_saved_floats: the save buffer's floats for fmt and M (-1: bad arguments). */
int64_t cn_field_train_saved_floats(int fmt, int64_t m);
int cn_radiance_field_train_fmt(int fmt, const float* packed, const float* code_bias, const int64_t* code_index,
                                int64_t n_codes, const float* pts, const float* ro, const float* rd,
                                const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                const float* freqs_xyz, const float* freqs_dir, float* raw, float* save,
                                uint32_t* masks, cn_stream_t stream);
int64_t cn_field_backward_train_workspace_floats(int64_t m);
int cn_field_backward_train(const float* packed_t, const float* const* params, const uint32_t* masks,
                            const float* saved, const float* x_enc, const float* d_raw, const float* pts,
                            const float* ro, const float* rd, const float* z, int64_t n_rays, int64_t n_samples,
                            int64_t chunk_rows, const int64_t* code_index, int64_t n_codes,
                            const float* freqs_xyz, const float* freqs_dir, float* workspace,
                            float* const* grads, float* g_code, float* d_pts, float* d_ro, float* d_rd,
                            cn_stream_t stream);
int cn_field_backward_train_fmt(int fmt_t, const float* packed_t, const float* const* params,
                                const uint32_t* masks, const float* saved, const float* x_enc, const float* d_raw,
                                const float* pts, const float* ro, const float* rd, const float* z, int64_t n_rays,
                                int64_t n_samples, int64_t chunk_rows, const int64_t* code_index, int64_t n_codes,
                                const float* freqs_xyz, const float* freqs_dir, float* workspace,
                                float* const* grads, float* g_code, float* d_pts, float* d_ro, float* d_rd,
                                cn_stream_t stream);
/* A render's fields' training backwards in shared launches (replaces two cn_field_backward_train_fmt
 * calls for predict_radiance_and_render's coarse and fine fields, nerf/__init__.py:81-89 under
 * train.py:112's loss.backward(): the fine depths are detached, point_sampler.py:115, so the two
 * backwards are independent).  Each field: the arguments of cn_field_backward_train_fmt, with its own
 * workspace (contents on entry are ignored).  With two fp32 fields on rays + depths that both take the
 * batched dW plan and the forward's encoding plane (every runnable training config): ONE dX launch, ONE
 * batched dW launch (layer_xyz1's dW among its jobs), ONE DIRS-pass launch and ONE reduction launch for
 * both, each running every field's workgroups as its own launch would -- the gradients are bitwise
 * those of the per-field calls.  Otherwise the fields run one after the other.  n_fields 1 or 2. */
typedef struct cn_field_train_bwd {
  const float* packed_t;
  const float* const* params;
  const uint32_t* masks;
  const float* saved;
  const float* x_enc;
  const float* d_raw;
  const float* pts;
  const float* ro;
  const float* rd;
  const float* z;
  int64_t n_rays, n_samples, chunk_rows;
  const int64_t* code_index;
  int64_t n_codes;
  const float* freqs_xyz;
  const float* freqs_dir;
  float* workspace;
  float* const* grads;
  float* g_code;
  float* d_pts;
  float* d_ro;
  float* d_rd;
} cn_field_train_bwd;
int cn_field_backward_train_multi(int fmt_t, const cn_field_train_bwd* fields, int n_fields, cn_stream_t stream);

/* Backward of cn_code_bias (the code layers, model.py:174-177, and the code
 * halves of layer_xyz2 / fc_out / fc_rgb) from g_code.  dz_s / dz_t (n_codes, 256)
 * are written (either may be NULL); grads as in cn_field_backward (accumulated). */
int cn_code_bias_backward(const float* const* params, const float* z_s, const float* z_t, int64_t n_codes,
                          const float* g_code, float* dz_s, float* dz_t, float* const* grads,
                          cn_stream_t stream);
/* The same backward in two launches with a caller-provided workspace
 * (cn_code_bias_backward_workspace_floats(n_codes) floats; contents on entry are ignored): each code's
 * layers and reductions are formed once, split over 64 workgroups, instead of once per workgroup.
 * Bitwise the same results as cn_code_bias_backward.  accumulate_dz = 1: dz_s / dz_t +=
 * the code gradients instead of = (the training step points them at the code tables'
 * gradient rows, so the coarse and fine fields' code gradients add up in place --
 * ShapeTextureEmbedding.forward in model.py:102-105 is the lookup they flow back to). */
int64_t cn_code_bias_backward_workspace_floats(int64_t n_codes);
/* The code backward on the forward's code-layer activations (code_act of cn_field_prepare_models),
 * first half: ds1 / ds2 / dt1 (ReLU-masked by code_act) into the workspace
 * (cn_code_bias_backward_workspace_floats; contents on entry are ignored; rows 3..5 of each code that
 * some sample used are written here, the rest stays as it was) and the code layers' / code halves'
 * parameter gradients added into grads (optional) -- no code layer is recomputed.  cn_code_dz forms dz
 * from it. */
int cn_code_bias_backward_act(const float* const* params, const float* z_s, const float* z_t, int64_t n_codes,
                              const float* code_act, const float* g_code, float* const* grads, float* workspace,
                              cn_stream_t stream);
/* cn_code_bias_backward_act of a render's 1 or 2 fields on the same codes in ONE launch (each job: the
 * arguments of one cn_code_bias_backward_act call; bitwise those calls' results). */
typedef struct cn_code_act_job {
  const float* const* params;
  const float* code_act;
  const float* g_code;
  float* const* grads;
  float* workspace;
} cn_code_act_job;
int cn_code_bias_backward_act_multi(const cn_code_act_job* jobs, int n_jobs, const float* z_s, const float* z_t,
                                    int64_t n_codes, cn_stream_t stream);
/* One field's part of cn_code_dz: its parameters, g_code and the workspace as cn_code_bias_backward_act
 * of the same field left it (only read: rows 3..5 of every code whose g_code row is not all zero). */
typedef struct cn_code_dz_job {
  const float* const* params;
  const float* g_code;
  const float* workspace;
} cn_code_dz_job;
/* dz_s / dz_t (n_codes, 256; either may be NULL) of 1 or 2 jobs on the same codes (a render's coarse and
 * fine fields, nerf/__init__.py:74-91), summed in job order; accumulate = 1: added to what dz holds. */
int cn_code_dz(const cn_code_dz_job* jobs, int n_jobs, int64_t n_codes, float* dz_s, float* dz_t, int accumulate,
               cn_stream_t stream);
int cn_code_bias_backward_ws(const float* const* params, const float* z_s, const float* z_t, int64_t n_codes,
                             const float* g_code, float* dz_s, float* dz_t, float* const* grads, float* workspace,
                             int accumulate_dz, cn_stream_t stream);

/* Backward of volume_render (volumetric_render.py:36-66) w.r.t. raw and rd
 * (z is detached in the reference).  Any of g_rgb (R,3), g_disp, g_acc, g_depth
 * (R), g_weights (R,S) may be NULL (zero).  d_raw (R,S,4) and d_rd (R,3, may be
 * NULL) are written -- d_rd added to instead with accumulate_rd = 1 (a running sum
 * of the rays' gradients over their consumers).  raw, z and d_raw 16-B aligned, or
 * CN_EINVAL. */
int cn_volume_render_backward(const float* raw, const float* z, const float* rd, int64_t n_rays,
                              int64_t n_samples, const float* g_rgb, const float* g_disp,
                              const float* g_acc, const float* g_weights, const float* g_depth,
                              float* d_raw, float* d_rd, int accumulate_rd, cn_stream_t stream);

/* Backward of get_bundle (ray_sampler.py:95-98): d_c2w (batch, 4, 4) rows 0..2
 * ACCUMULATED from g_ro / g_rd (batch*hw, 3), either may be NULL (not both). */
int cn_ray_bundle_backward(const float* dirs, int64_t hw, int64_t batch, const float* g_ro,
                           const float* g_rd, float* d_c2w, cn_stream_t stream);

/* Backward of the sample gather (ray_sampler.py:77-80): scatter-add g_ro / g_rd
 * (batch*sample_size, 3) into d_ro / d_rd (batch*hw, 3). */
int cn_gather_rays_backward(const float* g_ro, const float* g_rd, int64_t batch, int64_t hw,
                            const int64_t* select_inds, int64_t sample_size, float* d_ro, float* d_rd,
                            cn_stream_t stream);

/* Backward of cn_posenc (position_embed.py:35-53): dx (m, d) from g_enc (m, d*(inc + 2*num_freq)). */
int cn_posenc_backward(const float* x, int64_t m, int64_t d, const float* freqs, int64_t num_freq,
                       int include_input, const float* g_enc, float* dx, cn_stream_t stream);

/* Backward of cn_ray_points (z detached, point_sampler.py:115): d_ro += sum_s g_pts,
 * d_rd += sum_s g_pts * z; either output may be NULL (not both). */
int cn_ray_points_backward(const float* g_pts, const float* z, int64_t n_rays, int64_t n_samples,
                           float* d_ro, float* d_rd, cn_stream_t stream);

/* --- Scene composition, backward (fitting the poses and codes of posed objects) ---------
 * The four backwards around the compact fields of a scene render.  All are stream-ordered on `stream`, never
 * synchronise, use no float atomics and keep no state; argument errors return CN_EINVAL before any launch;
 * every element of every output is written. */

/* Backward of cn_volume_render_compose w.r.t. every object's raw rows and rd: the derivative of the
 * composition rule above read as real functions, with every sample's active set (and so its active count)
 * held fixed.  raws, z, rd and the sizes as the forward took them; g_rgb (R,3), g_disp, g_acc, g_depth (R),
 * g_weights (R,S), g_acc_objects (K,R): the upstream gradients, each may be NULL (zero).  Per sample, with
 * sigma_k, c_k, sigma, c and share_k as in the forward and w, T, sd, delta = dist |rd| of the integral:
 *   G_s = dL/dw_s = g_rgb . c_s + g_depth z_s + g_acc + g_w_s + sum_k g_acc_objects[k] share_k,s;
 *   dL/dsd_s = G_s T_s e^{-sd_s} - sum_{j>s} G_j w_j and d_rd = (sum_s dL/dsd_s sigma_s dist_s) rd / |rd|,
 *     g_disp folded into g_depth / g_acc: cn_volume_render_backward's arithmetic on sigma and c;
 *   with g_sigma = dL/dsd delta: an inactive object's row gets exactly (0, 0, 0, 0); the only active object a
 *     gets d c_a = w g_rgb and d sigma_a = g_sigma; with two or more active, d c_k = w g_rgb share_k and
 *     d sigma_k = g_sigma + sum_ch w g_rgb[ch] (c_k[ch] - c[ch]) / sigma
 *                         + sum_j w g_acc_objects[j] ((j == k) - share_j) / sigma;
 *   d raw_k = (d c_k 1.002 s (1 - s) per channel, s the channel's sigmoid; d sigma_k softplus20'(xs - 1), which
 *     is 1 above the threshold 20 and the sigmoid below).
 * With one object, or at a sample with one active object, and g_acc_objects NULL, the active row and d_rd are
 * cn_volume_render_backward's bits.  n_samples = 1 gives zeros.
 * d_raws: HOST array of n_objects device pointers, each (n_rays, n_samples, 4), 16-B aligned like every
 * raws[k] and z; d_rd (R,3) may be NULL, and is added to instead of written with accumulate_rd = 1.  One launch.
 * CN_EINVAL: raws, d_raws, an entry of either, z or rd NULL; n_objects outside 1..CN_MAX_SCENE_OBJECTS;
 * n_rays <= 0; n_samples outside 1..512; a misaligned tensor; accumulate_rd not 0 or 1. */
int cn_volume_render_compose_backward(const float* const* raws, int n_objects, const float* z, const float* rd,
                                      int64_t n_rays, int64_t n_samples, const float* g_rgb, const float* g_disp,
                                      const float* g_acc, const float* g_weights, const float* g_depth,
                                      const float* g_acc_objects, float* const* d_raws, float* d_rd,
                                      int accumulate_rd, cn_stream_t stream);

/* Floats of cn_object_rays_backward's workspace (its blocks' partial pose sums), or -1 for sizes it refuses. */
int64_t cn_object_rays_backward_workspace_floats(int64_t n_rays, int n_objects);

/* Backward of cn_object_rays: g_ro_obj, g_rd_obj (n_objects, n_rays, 3), either may be NULL (zero); ro, rd
 * and the HOST poses as the forward took them.  With R_k, t_k object k's rotation and translation:
 *   d_ro[r][j] = sum_k sum_i R_k[j][i] g_ro_obj[k][r][i], d_rd the same from g_rd_obj (ascending k, then i;
 *     one writer per element; added to the output instead with accumulate = 1);
 *   d_poses[k] (device, 12 floats: dR row-major, then dt), written:
 *     dR_k[j][i] = sum_r ((ro[r][j] - t_k[j]) g_ro_obj[k][r][i] + rd[r][j] g_rd_obj[k][r][i]),
 *     dt_k[j]    = - sum_r sum_i R_k[j][i] g_ro_obj[k][r][i].
 * The 12 sums per object are reduced in a fixed order (block partials in `workspace`, then one block per
 * object): two runs give the same bits.  d_ro, d_rd and d_poses may each be NULL (not all three); workspace:
 * cn_object_rays_backward_workspace_floats floats, contents on entry ignored, required with d_poses.  Two
 * launches (one without d_poses).
 * CN_EINVAL: ro, rd or poses NULL; no output; d_poses without a workspace; n_rays <= 0; n_objects outside
 * 1..CN_MAX_SCENE_OBJECTS; a pose entry that is not finite; accumulate not 0 or 1. */
int cn_object_rays_backward(const float* g_ro_obj, const float* g_rd_obj, const float* ro, const float* rd,
                            int64_t n_rays, const float* poses, int n_objects, float* d_ro, float* d_rd,
                            int accumulate, float* d_poses, float* workspace, cn_stream_t stream);

/* --- Scene composition with uniform scale, backward ----------------------
 * The two backwards above for similarity poses (the rule is beside cn_object_rays_scaled).  Stream-ordered, no
 * synchronisation, no float atomics, no state; every element of every output is written. */

/* Floats of cn_volume_render_compose_scaled_backward's workspace (its waves' partial scale sums), or -1 for
 * sizes it refuses. */
int64_t cn_volume_render_compose_scaled_backward_workspace_floats(int64_t n_rays, int64_t n_samples, int n_objects);

/* Backward of cn_volume_render_compose_scaled: cn_volume_render_compose_backward's derivative with sigma_k read
 * as the scaled density softplus20(xs - 1) / s_k.  With d sigma_k as defined there:
 *   d raw_k[3] = d sigma_k softplus20'(xs - 1) / s_k (the product, then the division);
 *   d_scales[k] = - sum_r sum_s d sigma_k[r][s] sigma_k[r][s] / s_k; an inactive slot contributes exactly 0.
 * d_scales: device, n_objects floats, written; may be NULL, and then no workspace is needed.  Its sums run in a
 * fixed order (a wave's lanes, then the waves' partials in `workspace`, one block per object): two runs give
 * the same bits.  One launch, two with d_scales.  With every scale 1 and d_scales NULL the outputs are
 * cn_volume_render_compose_backward's bits.
 * CN_EINVAL: what cn_volume_render_compose_backward refuses; scales NULL; a scale that is NaN, infinite or
 * <= 0; d_scales without a workspace. */
int cn_volume_render_compose_scaled_backward(const float* const* raws, const float* scales, int n_objects,
                                             const float* z, const float* rd, int64_t n_rays, int64_t n_samples,
                                             const float* g_rgb, const float* g_disp, const float* g_acc,
                                             const float* g_weights, const float* g_depth,
                                             const float* g_acc_objects, float* const* d_raws, float* d_rd,
                                             int accumulate_rd, float* d_scales, float* workspace,
                                             cn_stream_t stream);

/* Floats of cn_object_rays_scaled_backward's workspace, or -1 for sizes it refuses. */
int64_t cn_object_rays_scaled_backward_workspace_floats(int64_t n_rays, int n_objects);

/* Backward of cn_object_rays_scaled: cn_object_rays_backward with HOST poses of n_objects x 13 floats and
 * d_poses (device) n_objects x 13: dR, dt, ds.  With g' = g / s_k (g_ro_obj and g_rd_obj, the division rounded):
 *   d_ro, d_rd, dR_k, dt_k: cn_object_rays_backward's formulas on g';
 *   ds_k = - sum_r sum_i (ro_out[k][r][i] g_ro_obj[k][r][i] + rd_out[k][r][i] g_rd_obj[k][r][i]) / s_k, with
 *     ro_out, rd_out the forward's values, formed again;
 * the 13 sums per object reduced in cn_object_rays_backward's fixed order.  With every scale 1 the first 12
 * columns, d_ro and d_rd are cn_object_rays_backward's bits.
 * CN_EINVAL: what cn_object_rays_backward refuses; a scale that is NaN, infinite or <= 0. */
int cn_object_rays_scaled_backward(const float* g_ro_obj, const float* g_rd_obj, const float* ro, const float* rd,
                                   int64_t n_rays, const float* poses, int n_objects, float* d_ro, float* d_rd,
                                   int accumulate, float* d_poses, float* workspace, cn_stream_t stream);

/* Backward of cn_occupancy_expand: g_compact (M', 4) row j = g_raw (n_rays, n_samples, 4) row
 * sample_index[j]; the gradients of culled slots are dropped (the empty row is a constant).  workspace: what
 * the cull of the same sizes left, only read.  g_raw and g_compact 16-B aligned.  One launch.
 * CN_EINVAL: a pointer NULL; a size cn_occupancy_cull refuses; a misaligned tensor or workspace. */
int cn_occupancy_gather(const float* g_raw, const void* workspace, int64_t n_rays, int64_t n_samples,
                        float* g_compact, cn_stream_t stream);

/* Backward of the rows cn_occupancy_cull forms (z is not differentiated): g_pts, g_vdir (M', 3), either may be
 * NULL (zero) -> d_ro, d_rd (n_rays, 3), either may be NULL (not both), written.  fp32, every operation rounded:
 *   d_ro[r][i] = the sequential sum, from 0, over ray r's kept rows j in ascending order of g_pts[j][i];
 *   d_rd[r][i] = P + V, P the sequential sum over the same rows of z[r][s_j] * g_pts[j][i] (the product rounded),
 *     V the sequential sum of g_vdir[j][i] over the kept samples whose Q1 view-direction ray is r, in ascending
 *     sample index: with base and rcnt of r's chunk (cn_occupancy_cull, the same chunk_rows) these are the
 *     chunk's samples (r - base) + i rcnt, i = 0 .. n_samples - 1, sample k' being sample k' % n_samples of ray
 *     base + k' / n_samples.
 * A gather: one writer per element, a ray with nothing kept gets zeros.  workspace as cn_occupancy_gather.
 * One launch.
 * CN_EINVAL: z or workspace NULL; no output; a size cn_occupancy_cull refuses; chunk_rows <= 0; workspace not
 * 8-byte aligned. */
int cn_occupancy_cull_backward(const float* g_pts, const float* g_vdir, const float* z, const void* workspace,
                               int64_t n_rays, int64_t n_samples, int64_t chunk_rows, float* d_ro, float* d_rd,
                               cn_stream_t stream);

/* --- The step's scalar loss (train.py:103-108, eval.py:157-163) ---------------
 * out[6] = [mse(rgb_coarse, target[:, :3]), mse(rgb_fine, target[:, :3]),
 *           lambda * (||z_s|| + ||z_t||), their sum, ||z_s||, ||z_t||] (fp32, device), with
 * ||z|| = sqrt(expand * sum z^2) over n_code values (a code row expanded over `expand` rays,
 * eval; or whole tables with expand 1, train).  rgb_*: (n_rays, 3), either may be NULL;
 * target rows of target_stride floats (the first 3 are rgb).  n_code 0: no regulariser.
 * workspace: cn_render_loss_workspace_doubles(n_code) doubles (0: may be NULL) for the
 * multi-workgroup sums of large code tensors; contents on entry are ignored. */
int64_t cn_render_loss_workspace_doubles(int64_t n_code);
int cn_render_loss(const float* rgb_coarse, const float* rgb_fine, const float* target,
                   int64_t target_stride, int64_t n_rays, const float* z_s, const float* z_t,
                   int64_t n_code, int64_t expand, float regularizer_lambda, double* workspace, float* out,
                   cn_stream_t stream);
/* The same, plus psnr[0] = mse2psnr of the fine loss (of the coarse one without rgb_fine) in
 * float64 on the device -- utils/util.py:216-227 (-10 log10(mse), mse 0 -> 1e-5), the psnr
 * train.py:105 / eval.py:160 log -- so the caller needs no launches and no read-back for it. */
int cn_render_loss_psnr(const float* rgb_coarse, const float* rgb_fine, const float* target,
                        int64_t target_stride, int64_t n_rays, const float* z_s, const float* z_t,
                        int64_t n_code, int64_t expand, float regularizer_lambda, double* workspace,
                        float* out, double* psnr, cn_stream_t stream);
/* Its backward for an upstream gradient *grad_total (device scalar) of the sum, reading
 * the forward's out as stats: d_rgb_* (n_rays, 3) and d_z_* (n_code) WRITTEN (any NULL);
 * accumulate_z = 1: d_z_* added to (the codes' running gradient). */
int cn_render_loss_backward(const float* rgb_coarse, const float* rgb_fine, const float* target,
                            int64_t target_stride, int64_t n_rays, const float* z_s, const float* z_t,
                            int64_t n_code, int64_t expand, float regularizer_lambda, const float* stats,
                            const float* grad_total, float* d_rgb_coarse, float* d_rgb_fine, float* d_z_s,
                            float* d_z_t, int accumulate_z, cn_stream_t stream);

/* --- Training step: the optimiser (train.py:111-114, utils/util.py:147-172) ---
 * torch.optim.AdamW.step (decoupled weight decay; amsgrad / maximize off) over ONE
 * flat fp32 buffer holding every trained parameter, with its gradient and both
 * moments in three more buffers of the same layout (all 16-B aligned).  The update
 * runs over n_segments ranges [seg_begin[k], seg_end[k]) (HOST int64 arrays, float
 * offsets, multiples of 4, ascending, disjoint); segment k has its own lr[k],
 * weight_decay[k] (HOST double arrays) and step[k] (HOST int64, the step number
 * after this update, >= 1) -- normally one segment per param group; elements in no
 * segment are not touched.  Per element, in torch's _single_tensor_adam order with
 * each op rounded to fp32:
 *   p = p (1 - lr wd); m = lerp(m, g, 1 - beta1); v = v beta2 + ((1 - beta2) g) g;
 *   p = p + (-lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps). */
int cn_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_segments,
                  const int64_t* seg_begin, const int64_t* seg_end, const double* lr, const double* weight_decay,
                  const int64_t* step, double beta1, double beta2, double eps, cn_stream_t stream);

/* The same update with its per-segment scalars read from DEVICE memory, so a captured graph can
 * replay it with fresh ones: scalars = 3 floats per segment {1 - lr wd, -lr / (1 - beta1^step),
 * (1 - beta2^step)^0.5}, as cn_adamw_scalars folds them (host, the same double arithmetic as
 * cn_adamw_step).  Replaces optimizer.step() inside the captured eval iteration
 * (codenerf.evaluate.GraphedEvalStep; eval.py:165-167). */
int cn_adamw_scalars(int64_t n_segments, const double* lr, const double* weight_decay, const int64_t* step,
                     double beta1, double beta2, float* out);
int cn_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_segments,
                      const int64_t* seg_begin, const int64_t* seg_end, const float* scalars, double beta1,
                      double beta2, double eps, cn_stream_t stream);

/* fp32 MFMA GEMMs the backward is built from (row-major, leading dims in floats):
 *   cn_gemm_nn: C[M][N] = A[M][K] B[K][N], zeroed where mask[m][n] <= 0 (mask may be NULL); K <= 288;
 *   cn_gemm_tn: C[N][K] += sum_m A[M][N] B[M][K] (accumulates).
 * With ldc above the row length (and ldm above N) the columns between the rows are left as they are. */
int cn_gemm_nn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
               const float* mask, int64_t ldm, int64_t M, int64_t N, int64_t K, cn_stream_t stream);
int cn_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
               int64_t N, int64_t K, cn_stream_t stream);
/* The same two products as 3xbf16 (split operands on v_mfma_f32_32x32x16_bf16, fp32
 * accumulation; the GEMMs of cn_field_backward_fmt(CN_FMT_BF16X3)). */
int cn_gemm_nn_x3(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                  const float* mask, int64_t ldm, int64_t M, int64_t N, int64_t K, cn_stream_t stream);
int cn_gemm_tn_x3(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                  int64_t N, int64_t K, cn_stream_t stream);
/* cn_gemm_tn (fmt CN_FMT_F32) or cn_gemm_tn_x3 (CN_FMT_BF16X3), deterministic: each workgroup
 * stores its partial N x K tile into workspace (cn_gemm_tn_workspace_floats(M, N, K) floats; contents
 * on entry are ignored) and a second pass adds the partials to C in a fixed order, so the result is
 * bitwise reproducible (the float-atomic flush of cn_gemm_tn is not). */
int64_t cn_gemm_tn_workspace_floats(int64_t M, int64_t N, int64_t K);
int cn_gemm_tn_ws(int fmt, const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                  int64_t M, int64_t N, int64_t K, float* workspace, cn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CODENERF_H_ */
