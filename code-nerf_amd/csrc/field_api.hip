// The field's C entry points (include/codenerf.h): argument checks, kernel arguments, the launch.
// No kernel lives here -- the kernels and their launchers are mlp.hip (fp32 32x32x2), mlp_f32.hip
// (fp32 16x16x4), mlp_x3.hip and mlp_x3w.hip (3xbf16), mlp_f16.hip (fp16, inference only).  What the
// launchers share is in mlp_common.h (the mode dispatch) and cn_common.h (the persistent grid); what
// the streamed kernels share is in mlp_stream.h.
//
// Every entry that takes a field call's geometry, codes and frequency tables gets their checks and its
// FieldArgs from field_args (encoded rows: encoded_args) and states only what is its own: its buffers,
// its format rule and the launch.  A new entry point does the same.
#include "mlp_common.h"

using namespace cn::mlp;

namespace cn {
namespace mlp {

// m's bound at every entry: the workgroups of a 128-sample tile (mlp.hip, mlp_x3.hip) fit an int
constexpr int kTile = 128;

int field_args(const FieldInputs& in, FieldForm form, int wave_samples, FieldArgs& a) {
  const bool density = form == kDensityForm, encode = form == kEncodeForm;
  CN_CHECK_ARG(in.freqs_xyz && (density || in.freqs_dir));
  if (density) {
    const bool rays = in.ro || in.rd || in.z;
    CN_CHECK_ARG((in.pts ? 1 : 0) + (rays ? 1 : 0) + (in.x ? 1 : 0) == 1);  // exactly one input mode
    CN_CHECK_ARG(!rays || (in.ro && in.rd && in.z));
  } else {
    CN_CHECK_ARG(in.rd && (in.pts || (in.ro && in.z)));
  }
  CN_CHECK_ARG(in.n_rays > 0 && in.n_samples > 0 && (density || in.chunk_rows > 0));
  CN_CHECK_ARG(in.n_rays <= INT64_MAX / in.n_samples);  // m below cannot overflow
  if (!encode) {
    CN_CHECK_ARG(in.n_codes > 0 && (in.code_index || in.n_codes == 1 || in.n_codes == in.n_rays));
    if (wave_samples && !(in.n_codes == 1 || in.n_samples % wave_samples == 0)) return CN_EUNSUPPORTED;
    CN_CHECK_ARG(cn::ceil_div(in.n_rays * in.n_samples, kTile) <= 0x7fffffff);
  }
  a = FieldArgs{};
  if (!encode) {
    a.code_index = in.code_index;
    a.n_codes = in.n_codes;
  }
  a.pts = in.pts;
  a.ro = in.ro;
  a.rd = in.rd;
  a.z = in.z;
  a.x = density ? in.x : nullptr;
  a.n_rays = in.n_rays;
  a.n_samples = in.n_samples;
  a.chunk_rows = density ? in.n_rays : in.chunk_rows;
  a.m = in.n_rays * in.n_samples;
  for (int i = 0; i < 10; ++i) a.fx[i] = in.freqs_xyz[i];
  if (!density)
    for (int i = 0; i < 4; ++i) a.fd[i] = in.freqs_dir[i];
  return CN_OK;
}

int encoded_args(const float* x, int64_t m, const int64_t* code_index, int64_t n_codes, FieldArgs& a) {
  CN_CHECK_ARG(x && m > 0 && n_codes > 0);
  CN_CHECK_ARG(code_index || n_codes == 1 || n_codes == m);
  CN_CHECK_ARG(cn::ceil_div(m, kTile) <= 0x7fffffff);
  a = FieldArgs{};
  a.code_index = code_index;
  a.n_codes = n_codes;
  a.x = x;
  a.m = m;
  return CN_OK;
}

int fused_backward_args(int fmt_t, const cn_field_fused_bwd& f, FieldArgs& a) {
  CN_CHECK_ARG(fmt_t == CN_FMT_BF16X3_T || fmt_t == CN_FMT_F32_W16_T);
  CN_CHECK_ARG(f.packed_t && f.masks && f.d_raw && f.g_code);
  CN_CHECK_ARG(!f.d_pts || f.pts);
  CN_CHECK_ARG(!f.d_ro || (f.ro && f.z && !f.pts));
  // one code row per wave (32 samples x3, 16 samples w16): a single code, or every wave inside one ray
  const FieldInputs in = {f.pts,        f.ro,         f.rd,      f.z,         f.n_rays,   f.n_samples,
                          f.chunk_rows, f.code_index, f.n_codes, f.freqs_xyz, f.freqs_dir};
  CN_TRY(field_args(in, kRayForm, fmt_t == CN_FMT_BF16X3_T ? 32 : 16, a));
  CN_CHECK_ARG(cn::aligned16(f.d_raw));  // float4 rows (include/codenerf.h)
  a.packed = f.packed_t;
  a.masks = const_cast<uint32_t*>(f.masks);
  a.d_raw = f.d_raw;
  a.g_code = f.g_code;
  a.d_pts = f.d_pts;
  a.d_ro = f.d_ro;
  a.d_rd = f.d_rd;
  return CN_OK;
}

}  // namespace mlp
}  // namespace cn

namespace {

int make_params(const float* const* params, Params* P) {
  if (!params) return CN_EINVAL;
  for (int i = 0; i < CN_NUM_PARAMS; ++i) {
    if (!params[i]) return CN_EINVAL;
    P->p[i] = params[i];
  }
  return CN_OK;
}

bool valid_fmt(int fmt) {
  return fmt == CN_FMT_F32 || fmt == CN_FMT_BF16X3 || fmt == CN_FMT_F32_W16 || fmt == CN_FMT_BF16X3_W16 ||
         fmt == CN_FMT_F16;
}
bool valid_pack_fmt(int fmt) {
  return valid_fmt(fmt) || fmt == CN_FMT_BF16X3_T || fmt == CN_FMT_F32_W16_T || fmt == CN_FMT_F32_W16_FOLD;
}

// fmt at a forward entry point: the folded pack runs through the *_fold entry points only, and they
// take no other (CN_EUNSUPPORTED, before any other check and without a launch).
int forward_fmt_status(int fmt, bool fold_entry) {
  if (!(valid_fmt(fmt) || fmt == CN_FMT_F32_W16_FOLD)) return CN_EINVAL;
  return (fmt == CN_FMT_F32_W16_FOLD) == fold_entry ? CN_OK : CN_EUNSUPPORTED;
}

int launch_field(int fmt, int mode, FieldArgs& a, hipStream_t st) {
  if (fmt == CN_FMT_BF16X3) return launch_field_x3(mode, a, st);
  if (fmt == CN_FMT_F32_W16) return launch_field_w16(mode, a, st);
  if (fmt == CN_FMT_BF16X3_W16) return launch_field_x3w(mode, a, st);
  if (fmt == CN_FMT_F32_W16_FOLD) return launch_field_w16_fold(mode, a, st);
  if (fmt == CN_FMT_F16) return launch_field_f16(mode, a, st);
  return launch_field_v1(mode, a, st);
}

int geometry_mode(const FieldArgs& a) { return a.pts ? kFromPts : (a.x ? kFromEncoded : kFromRayZ); }

// What every forward over points or rays takes besides its inputs: the pack, the code rows, the output.
int forward_args(const FieldInputs& in, const float* packed, const float* code_bias, float* raw, FieldArgs& a) {
  CN_CHECK_ARG(packed && code_bias && raw && cn::aligned16(raw));  // float4 rows (include/codenerf.h)
  CN_TRY(field_args(in, kRayForm, 0, a));
  a.packed = packed;
  a.code_bias = code_bias;
  a.raw = raw;
  return CN_OK;
}

// cn_mlp_forward / cn_mlp_forward_fold (fold_entry: fold_bias required)
int mlp_forward_any(const float* packed, int fmt, bool fold_entry, const float* code_bias, const float* fold_bias,
                    const int64_t* code_index, int64_t n_codes, const float* x, int64_t m, float* raw,
                    cn_stream_t stream) {
  CN_TRY(forward_fmt_status(fmt, fold_entry));
  CN_CHECK_ARG(packed && code_bias && raw && (!fold_entry || fold_bias));
  CN_CHECK_ARG(cn::aligned16(raw));        // float4 rows (include/codenerf.h)
  CN_CHECK_ARG(cn::aligned16(fold_bias));  // 16-B vector reads of a c_v1 row
  FieldArgs a;
  CN_TRY(encoded_args(x, m, code_index, n_codes, a));
  a.packed = packed;
  a.code_bias = code_bias;
  a.fold_bias = fold_bias;
  a.raw = raw;
  return launch_field(fmt, kFromEncoded, a, cn::as_stream(stream));
}

// cn_radiance_field / cn_radiance_field_fold
int radiance_field_any(const float* packed, int fmt, bool fold_entry, const float* code_bias, const float* fold_bias,
                       const FieldInputs& in, float* raw, cn_stream_t stream) {
  CN_TRY(forward_fmt_status(fmt, fold_entry));
  CN_CHECK_ARG(!fold_entry || fold_bias);
  CN_CHECK_ARG(cn::aligned16(fold_bias));  // 16-B vector reads of a c_v1 row
  FieldArgs a;
  CN_TRY(forward_args(in, packed, code_bias, raw, a));
  a.fold_bias = fold_bias;
  return launch_field(fmt, geometry_mode(a), a, cn::as_stream(stream));
}

// What the counted entries add to their parents' rules (include/codenerf.h): the one format, the points
// form with one sample per row, codes by one row or code_index, and the device row count.
int counted_status(int fmt, int want_fmt, const float* pts, const float* ro, const float* z, int64_t n_rows_max,
                   int64_t n_samples, const int64_t* code_index, int64_t n_codes, const int64_t* count) {
  CN_CHECK_ARG(fmt == want_fmt);
  CN_CHECK_ARG(pts && !ro && !z && n_samples == 1 && n_rows_max > 0);
  CN_CHECK_ARG(code_index || n_codes == 1);
  CN_CHECK_ARG(count && (reinterpret_cast<uintptr_t>(count) & 7) == 0);
  return CN_OK;
}

// cn_radiance_field_counted / cn_radiance_field_fold_counted
int radiance_field_counted_any(const float* packed, int fmt, bool fold_entry, const float* code_bias,
                               const float* fold_bias, const int64_t* code_index, int64_t n_codes, const float* pts,
                               const float* ro, const float* rd, const float* z, int64_t n_rows_max, int64_t n_samples,
                               const int64_t* count, const float* freqs_xyz, const float* freqs_dir, float* raw,
                               cn_stream_t stream) {
  CN_TRY(counted_status(fmt, fold_entry ? CN_FMT_F32_W16_FOLD : CN_FMT_F32_W16, pts, ro, z, n_rows_max, n_samples,
                        code_index, n_codes, count));
  CN_CHECK_ARG(!fold_entry || fold_bias);
  CN_CHECK_ARG(cn::aligned16(fold_bias));  // 16-B vector reads of a c_v1 row
  // the capacity as n_rays = chunk_rows: with one sample per row the Q1 ray is the row itself
  const FieldInputs in = {pts, nullptr, rd, nullptr, n_rows_max, 1, n_rows_max, code_index, n_codes, freqs_xyz,
                          freqs_dir};
  FieldArgs a;
  CN_TRY(forward_args(in, packed, code_bias, raw, a));
  a.fold_bias = fold_bias;
  return launch_field_w16_counted(fold_entry, a, count, cn::as_stream(stream));
}

}  // namespace

extern "C" int64_t cn_mlp_packed_floats(int fmt) {
  if (!valid_pack_fmt(fmt)) return -1;
  if (fmt == CN_FMT_F32_W16 || fmt == CN_FMT_F32_W16_T) return packed_floats_w16();
  if (fmt == CN_FMT_F32_W16_FOLD) return packed_floats_w16_fold();
  if (fmt == CN_FMT_BF16X3_W16) return packed_floats_x3w();
  if (fmt == CN_FMT_F16) return packed_floats_f16();
  return fmt == CN_FMT_F32 ? kPackedFloats : packed_floats_x3();
}

extern "C" int cn_mlp_pack(const float* const* params, int fmt, float* packed, cn_stream_t stream) {
  Params P;
  if (make_params(params, &P) != CN_OK || !packed || !valid_pack_fmt(fmt)) return CN_EINVAL;
  if (fmt == CN_FMT_BF16X3) return launch_pack_x3(P, packed, cn::as_stream(stream));
  if (fmt == CN_FMT_BF16X3_T) return launch_pack_x3t(P, packed, cn::as_stream(stream));
  if (fmt == CN_FMT_F32_W16) return launch_pack_w16(P, packed, cn::as_stream(stream));
  if (fmt == CN_FMT_F32_W16_T) return launch_pack_w16t(P, packed, cn::as_stream(stream));
  if (fmt == CN_FMT_F32_W16_FOLD) return launch_pack_w16_fold(P, packed, cn::as_stream(stream));
  if (fmt == CN_FMT_BF16X3_W16) return launch_pack_x3w(P, packed, cn::as_stream(stream));
  if (fmt == CN_FMT_F16) return launch_pack_f16(P, packed, cn::as_stream(stream));
  return launch_pack_v1(P, packed, cn::as_stream(stream));
}

extern "C" int cn_code_bias(const float* const* params, const float* z_s, const float* z_t,
                            int64_t n_codes, float* code_bias, cn_stream_t stream) {
  Params P;
  if (make_params(params, &P) != CN_OK) return CN_EINVAL;
  CN_CHECK_ARG(z_s && z_t && code_bias && n_codes > 0 && n_codes * kCbSlices <= (1ll << 31) - 1);
  return launch_code_bias(P, z_s, z_t, n_codes, code_bias, cn::as_stream(stream));
}

extern "C" int cn_fold_bias(const float* const* params, const float* code_bias, int64_t n_codes, float* fold_bias,
                            cn_stream_t stream) {
  Params P;
  if (make_params(params, &P) != CN_OK) return CN_EINVAL;
  CN_CHECK_ARG(code_bias && fold_bias && n_codes > 0 && n_codes * kFbSlices <= (1ll << 31) - 1);
  return launch_fold_bias(P, code_bias, n_codes, fold_bias, cn::as_stream(stream));
}

extern "C" int cn_field_prepare(const float* const* params, const float* z_s, const float* z_t, int64_t n_codes,
                                float* code_bias, float* packed, float* packed_t, float* zero, int64_t n_zero,
                                cn_stream_t stream) {
  const cn_field_prep m = {params, code_bias, packed, packed_t, zero, n_zero, nullptr};
  return cn_field_prepare_models(&m, 1, z_s, z_t, n_codes, stream);
}

extern "C" int cn_field_prepare_models(const cn_field_prep* models, int n_models, const float* z_s, const float* z_t,
                                       int64_t n_codes, cn_stream_t stream) {
  CN_CHECK_ARG(models && n_models >= 1 && n_models <= 2);
  PrepareModel pm[2];
  for (int k = 0; k < n_models; ++k) {
    const cn_field_prep& m = models[k];
    if (make_params(m.params, &pm[k].P) != CN_OK) return CN_EINVAL;
    CN_CHECK_ARG(m.n_zero >= 0 && (m.n_zero == 0 || m.zero));
    CN_CHECK_ARG(!m.code_bias || (z_s && z_t && n_codes > 0 && n_codes * kCbSlices + 256 <= 0x7fffffff));
    CN_CHECK_ARG(!m.code_act || m.code_bias);
    pm[k].code_bias = m.code_bias;
    pm[k].code_act = m.code_act;
    pm[k].packed = m.packed;
    pm[k].packed_t = m.packed_t;
    pm[k].zero = m.zero;
    pm[k].n_zero = m.n_zero;
  }
  return launch_field_prepare_w16(pm, n_models, z_s, z_t, n_codes, cn::as_stream(stream));
}

extern "C" int cn_mlp_forward(const float* packed, int fmt, const float* code_bias,
                              const int64_t* code_index, int64_t n_codes, const float* x,
                              int64_t m, float* raw, cn_stream_t stream) {
  return mlp_forward_any(packed, fmt, false, code_bias, nullptr, code_index, n_codes, x, m, raw, stream);
}

extern "C" int cn_mlp_forward_fold(const float* packed, int fmt, const float* code_bias, const float* fold_bias,
                                   const int64_t* code_index, int64_t n_codes, const float* x, int64_t m,
                                   float* raw, cn_stream_t stream) {
  return mlp_forward_any(packed, fmt, true, code_bias, fold_bias, code_index, n_codes, x, m, raw, stream);
}

extern "C" int cn_radiance_field(const float* packed, int fmt, const float* code_bias,
                                 const int64_t* code_index, int64_t n_codes, const float* pts,
                                 const float* ro, const float* rd, const float* z, int64_t n_rays,
                                 int64_t n_samples, int64_t chunk_rows, const float* freqs_xyz,
                                 const float* freqs_dir, float* raw, cn_stream_t stream) {
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, chunk_rows, code_index, n_codes, freqs_xyz, freqs_dir};
  return radiance_field_any(packed, fmt, false, code_bias, nullptr, in, raw, stream);
}

extern "C" int cn_radiance_field_fold(const float* packed, int fmt, const float* code_bias, const float* fold_bias,
                                      const int64_t* code_index, int64_t n_codes, const float* pts,
                                      const float* ro, const float* rd, const float* z, int64_t n_rays,
                                      int64_t n_samples, int64_t chunk_rows, const float* freqs_xyz,
                                      const float* freqs_dir, float* raw, cn_stream_t stream) {
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, chunk_rows, code_index, n_codes, freqs_xyz, freqs_dir};
  return radiance_field_any(packed, fmt, true, code_bias, fold_bias, in, raw, stream);
}

extern "C" int cn_radiance_field_counted(const float* packed, int fmt, const float* code_bias,
                                         const int64_t* code_index, int64_t n_codes, const float* pts,
                                         const float* ro, const float* rd, const float* z, int64_t n_rows_max,
                                         int64_t n_samples, const int64_t* count, const float* freqs_xyz,
                                         const float* freqs_dir, float* raw, cn_stream_t stream) {
  return radiance_field_counted_any(packed, fmt, false, code_bias, nullptr, code_index, n_codes, pts, ro, rd, z,
                                    n_rows_max, n_samples, count, freqs_xyz, freqs_dir, raw, stream);
}

extern "C" int cn_radiance_field_fold_counted(const float* packed, int fmt, const float* code_bias,
                                              const float* fold_bias, const int64_t* code_index, int64_t n_codes,
                                              const float* pts, const float* ro, const float* rd, const float* z,
                                              int64_t n_rows_max, int64_t n_samples, const int64_t* count,
                                              const float* freqs_xyz, const float* freqs_dir, float* raw,
                                              cn_stream_t stream) {
  return radiance_field_counted_any(packed, fmt, true, code_bias, fold_bias, code_index, n_codes, pts, ro, rd, z,
                                    n_rows_max, n_samples, count, freqs_xyz, freqs_dir, raw, stream);
}

extern "C" int64_t cn_view_rows_bytes(int64_t n_rays) {
  return (n_rays > 0 && n_rays <= INT64_MAX / (kHidden * 4)) ? n_rays * kHidden * 4 : -1;
}

extern "C" int cn_view_rows(const float* packed, int fmt, const float* fold_bias, const float* rd, int64_t n_rays,
                            const float* freqs_dir, float* view_rows, cn_stream_t stream) {
  CN_TRY(forward_fmt_status(fmt, true));
  CN_CHECK_ARG(packed && fold_bias && rd && freqs_dir && view_rows);
  CN_CHECK_ARG(n_rays > 0 && cn_view_rows_bytes(n_rays) > 0);
  CN_CHECK_ARG(cn::aligned16(packed) && cn::aligned16(fold_bias) && cn::aligned16(view_rows));  // 16-B vector accesses
  FieldArgs a = {};
  a.packed = packed;
  a.fold_bias = fold_bias;
  a.rd = rd;
  a.n_rays = n_rays;
  for (int i = 0; i < 4; ++i) a.fd[i] = freqs_dir[i];
  return launch_view_rows_w16(a, view_rows, cn::as_stream(stream));
}

extern "C" int cn_radiance_field_fold_rows(const float* packed, int fmt, const float* code_bias,
                                           const float* fold_bias, const float* view_rows,
                                           const int64_t* code_index, int64_t n_codes, const float* pts,
                                           const float* ro, const float* rd, const float* z, int64_t n_rays,
                                           int64_t n_samples, int64_t chunk_rows, const float* freqs_xyz,
                                           const float* freqs_dir, float* raw, cn_stream_t stream) {
  CN_TRY(forward_fmt_status(fmt, true));
  CN_CHECK_ARG(fold_bias && view_rows && cn::aligned16(fold_bias) && cn::aligned16(view_rows));
  CN_CHECK_ARG(n_codes == 1 && !code_index);  // the rows hold code row 0's c_v1
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, chunk_rows, nullptr, 1, freqs_xyz, freqs_dir};
  FieldArgs a;
  CN_TRY(forward_args(in, packed, code_bias, raw, a));
  CN_CHECK_ARG(cn_view_rows_bytes(n_rays) > 0);
  a.fold_bias = fold_bias;
  a.view_rows = view_rows;
  return launch_field_w16_fold_rows(geometry_mode(a), a, cn::as_stream(stream));
}

extern "C" int cn_density_field(const float* packed, int fmt, const float* code_bias, const int64_t* code_index,
                                int64_t n_codes, const float* pts, const float* ro, const float* rd, const float* z,
                                const float* x, int64_t x_stride, int64_t n_rays, int64_t n_samples,
                                const float* freqs_xyz, float* sigma, float* raw, cn_stream_t stream) {
  CN_CHECK_ARG(packed && code_bias && (sigma || raw));
  CN_CHECK_ARG(cn::aligned16(raw));  // float4 rows (include/codenerf.h)
  CN_CHECK_ARG(!x || x_stride >= kDimXyz);
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, 0, code_index, n_codes, freqs_xyz, nullptr, x};
  DensityArgs d = {};
  CN_TRY(field_args(in, kDensityForm, 0, d.f));
  if (fmt != CN_FMT_F32_W16) return (valid_fmt(fmt) || fmt == CN_FMT_F32_W16_FOLD) ? CN_EUNSUPPORTED : CN_EINVAL;
  d.f.packed = packed;
  d.f.code_bias = code_bias;
  d.f.raw = raw;
  d.sigma = sigma;
  d.x_stride = x_stride;
  return launch_density_w16(geometry_mode(d.f), d, cn::as_stream(stream));
}

extern "C" int cn_density_field_counted(const float* packed, int fmt, const float* code_bias,
                                        const int64_t* code_index, int64_t n_codes, const float* pts, const float* ro,
                                        const float* rd, const float* z, int64_t n_rows_max, int64_t n_samples,
                                        const int64_t* count, const float* freqs_xyz, float* sigma, float* raw,
                                        cn_stream_t stream) {
  CN_TRY(counted_status(fmt, CN_FMT_F32_W16, pts, ro, z, n_rows_max, n_samples, code_index, n_codes, count));
  CN_CHECK_ARG(!rd && packed && code_bias && (sigma || raw));
  CN_CHECK_ARG(cn::aligned16(raw));  // float4 rows (include/codenerf.h)
  const FieldInputs in = {pts, nullptr, nullptr, nullptr, n_rows_max, 1, 0, code_index, n_codes, freqs_xyz, nullptr,
                          nullptr};
  DensityArgs d = {};
  CN_TRY(field_args(in, kDensityForm, 0, d.f));
  d.f.packed = packed;
  d.f.code_bias = code_bias;
  d.f.raw = raw;
  d.sigma = sigma;
  return launch_density_w16_counted(d, count, cn::as_stream(stream));
}

extern "C" int cn_density_gradient(const float* packed, const float* packed_t, int fmt, int fmt_t,
                                   const float* code_bias, const int64_t* code_index, int64_t n_codes,
                                   const float* pts, const float* ro, const float* rd, const float* z, int64_t n_rays,
                                   int64_t n_samples, const float* freqs_xyz, float* grad_sigma,
                                   cn_stream_t stream) {
  CN_CHECK_ARG(packed && packed_t && code_bias && grad_sigma);
  CN_CHECK_ARG(cn::aligned16(grad_sigma));  // float4 rows (include/codenerf.h)
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, 0, code_index, n_codes, freqs_xyz, nullptr};
  DensityArgs d = {};
  CN_TRY(field_args(in, kDensityForm, 0, d.f));
  // fmt a forward format, fmt_t a transposed one (the two swapped, or an unknown value: invalid)
  CN_CHECK_ARG(valid_fmt(fmt) || fmt == CN_FMT_F32_W16_FOLD);
  CN_CHECK_ARG(fmt_t == CN_FMT_BF16X3_T || fmt_t == CN_FMT_F32_W16_T);
  if (fmt != CN_FMT_F32_W16 || fmt_t != CN_FMT_F32_W16_T) return CN_EUNSUPPORTED;
  d.f.packed = packed;
  d.f.code_bias = code_bias;
  d.f.raw = grad_sigma;
  return launch_density_grad_w16(geometry_mode(d.f), d, packed_t, cn::as_stream(stream));
}

extern "C" int cn_radiance_field_train(const float* packed, const float* code_bias, const int64_t* code_index,
                                       int64_t n_codes, const float* pts, const float* ro, const float* rd,
                                       const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                       const float* freqs_xyz, const float* freqs_dir, float* raw, float* save,
                                       cn_stream_t stream) {
  CN_CHECK_ARG(save);
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, chunk_rows, code_index, n_codes, freqs_xyz, freqs_dir};
  FieldArgs a;
  CN_TRY(forward_args(in, packed, code_bias, raw, a));
  a.save = save;
  return launch_field_v1(geometry_mode(a), a, cn::as_stream(stream));
}

extern "C" int cn_mlp_forward_train(const float* packed, const float* code_bias, const int64_t* code_index,
                                    int64_t n_codes, const float* x, int64_t m, float* raw, float* save,
                                    cn_stream_t stream) {
  CN_CHECK_ARG(packed && code_bias && raw && save);
  CN_CHECK_ARG(cn::aligned16(raw));  // float4 rows (include/codenerf.h)
  FieldArgs a;
  CN_TRY(encoded_args(x, m, code_index, n_codes, a));
  a.packed = packed;
  a.code_bias = code_bias;
  a.raw = raw;
  a.save = save;
  return launch_field_v1(kFromEncoded, a, cn::as_stream(stream));
}

extern "C" int64_t cn_field_mask_words(int64_t m) { return m > 0 ? mask_words_x3(m) : -1; }

extern "C" int64_t cn_field_mask_words_fmt(int fmt, int64_t m) {
  if (m <= 0) return -1;
  if (fmt == CN_FMT_BF16X3) return mask_words_x3(m);
  if (fmt == CN_FMT_F32_W16) return mask_words_w16(m);
  return -1;
}

extern "C" int cn_radiance_field_masks(const float* packed, const float* code_bias, const int64_t* code_index,
                                       int64_t n_codes, const float* pts, const float* ro, const float* rd,
                                       const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                       const float* freqs_xyz, const float* freqs_dir, float* raw, uint32_t* masks,
                                       cn_stream_t stream) {
  return cn_radiance_field_masks_fmt(CN_FMT_BF16X3, packed, code_bias, code_index, n_codes, pts, ro, rd, z, n_rays,
                                     n_samples, chunk_rows, freqs_xyz, freqs_dir, raw, masks, stream);
}

extern "C" int cn_radiance_field_masks_fmt(int fmt, const float* packed, const float* code_bias,
                                           const int64_t* code_index, int64_t n_codes, const float* pts,
                                           const float* ro, const float* rd, const float* z, int64_t n_rays,
                                           int64_t n_samples, int64_t chunk_rows, const float* freqs_xyz,
                                           const float* freqs_dir, float* raw, uint32_t* masks, cn_stream_t stream) {
  CN_CHECK_ARG((fmt == CN_FMT_BF16X3 || fmt == CN_FMT_F32_W16) && masks);
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, chunk_rows, code_index, n_codes, freqs_xyz, freqs_dir};
  FieldArgs a;
  CN_TRY(forward_args(in, packed, code_bias, raw, a));
  a.masks = masks;
  return launch_field(fmt, geometry_mode(a), a, cn::as_stream(stream));
}

extern "C" int cn_radiance_field_train_w16(const float* packed, const float* code_bias, const int64_t* code_index,
                                           int64_t n_codes, const float* pts, const float* ro, const float* rd,
                                           const float* z, int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                           const float* freqs_xyz, const float* freqs_dir, float* raw, float* save,
                                           uint32_t* masks, cn_stream_t stream) {
  return cn_radiance_field_train_fmt(CN_FMT_F32_W16, packed, code_bias, code_index, n_codes, pts, ro, rd, z, n_rays,
                                     n_samples, chunk_rows, freqs_xyz, freqs_dir, raw, save, masks, stream);
}

extern "C" int cn_radiance_field_train_fmt(int fmt, const float* packed, const float* code_bias,
                                           const int64_t* code_index, int64_t n_codes, const float* pts,
                                           const float* ro, const float* rd, const float* z, int64_t n_rays,
                                           int64_t n_samples, int64_t chunk_rows, const float* freqs_xyz,
                                           const float* freqs_dir, float* raw, float* save, uint32_t* masks,
                                           cn_stream_t stream) {
  CN_CHECK_ARG((fmt == CN_FMT_F32_W16 || fmt == CN_FMT_BF16X3) && save && masks);
  const FieldInputs in = {pts, ro, rd, z, n_rays, n_samples, chunk_rows, code_index, n_codes, freqs_xyz, freqs_dir};
  FieldArgs a;
  CN_TRY(forward_args(in, packed, code_bias, raw, a));
  a.save = save;
  a.masks = masks;
  // fp32: the encoding plane follows the five activation planes (cn_field_train_saved_floats)
  if (fmt == CN_FMT_F32_W16) a.xenc = save + 5 * a.m * 256;
  return launch_field(fmt, geometry_mode(a), a, cn::as_stream(stream));
}

extern "C" int64_t cn_field_train_saved_floats(int fmt, int64_t m) {
  if (m <= 0 || !(fmt == CN_FMT_F32_W16 || fmt == CN_FMT_BF16X3)) return -1;
  // five (m, 256) activation planes; fp32: then the (m, 64) encoding plane; a 256-float scratch row
  return 5 * m * 256 + (fmt == CN_FMT_F32_W16 ? 64 * m : 0) + 256;
}

extern "C" int cn_field_backward_x3(const float* packed_t, const uint32_t* masks, const float* d_raw,
                                    const float* pts, const float* ro, const float* rd, const float* z,
                                    int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                    const int64_t* code_index, int64_t n_codes, const float* freqs_xyz,
                                    const float* freqs_dir, float* g_code, float* d_pts, float* d_ro, float* d_rd,
                                    cn_stream_t stream) {
  return cn_field_backward_fused(CN_FMT_BF16X3_T, packed_t, masks, d_raw, pts, ro, rd, z, n_rays, n_samples,
                                 chunk_rows, code_index, n_codes, freqs_xyz, freqs_dir, g_code, d_pts, d_ro, d_rd,
                                 stream);
}

extern "C" int cn_field_backward_fused(int fmt_t, const float* packed_t, const uint32_t* masks, const float* d_raw,
                                       const float* pts, const float* ro, const float* rd, const float* z,
                                       int64_t n_rays, int64_t n_samples, int64_t chunk_rows,
                                       const int64_t* code_index, int64_t n_codes, const float* freqs_xyz,
                                       const float* freqs_dir, float* g_code, float* d_pts, float* d_ro,
                                       float* d_rd, cn_stream_t stream) {
  const cn_field_fused_bwd f = {packed_t, masks, d_raw, pts, ro, rd, z, n_rays, n_samples, chunk_rows, code_index,
                                n_codes, freqs_xyz, freqs_dir, g_code, d_pts, d_ro, d_rd, nullptr};
  FieldArgs a;
  CN_TRY(fused_backward_args(fmt_t, f, a));
  return fmt_t == CN_FMT_BF16X3_T ? launch_field_x3_bwd(geometry_mode(a), a, cn::as_stream(stream))
                                  : launch_field_w16_bwd(geometry_mode(a), a, cn::as_stream(stream));
}
