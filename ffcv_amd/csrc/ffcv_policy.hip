// ffcv_policy.hip -- the draws of TrivialAugmentWide: which
// of 14 operations a sample runs and at what strength (op id 20), turned into
// the per-sample arguments of the pixel launches that follow
// (ffcv_color_jitter_batch twice, ffcv_tone_batch_bits, ffcv_affine_batch,
// ffcv_sharpness_batch).  One lane per sample; the host twin runs the same
// function.  No pixel is touched here.
#include "affine_common.h"
#include "api_internal.h"
#include "color_common.h"

#define FFCV_POLICY_OP 20
#define FFCV_POLICY_NOPS 14

// the 14 operations, in the order of the value table's rows
enum {
  POL_IDENTITY = 0, POL_SHEAR_X, POL_SHEAR_Y, POL_TRANSLATE_X, POL_TRANSLATE_Y, POL_ROTATE, POL_BRIGHTNESS, POL_COLOR,
  POL_CONTRAST, POL_SHARPNESS, POL_POSTERIZE, POL_SOLARIZE, POL_AUTOCONTRAST, POL_EQUALIZE
};

struct PolicyOut {
  uint8_t *op, *cj_apply;
  double *cj_ratio;
  uint8_t *tone_apply, *tone_bits, *aff_apply;
  int64_t *aff_coef;
  uint8_t *sharp_apply;
  float *sharp_factor;
};

// One sample's three draws, always all three, and every launch's arguments
// for it.  Returns 1 when the MT19937 stream ran out.
FFCV_HD int draw_policy(int k, int B, uint64_t id, uint64_t loader_seed, uint64_t epoch, int nbins,
                         const double *table, int H, int W, const PolicyOut &o) {
  DevMT m;
  mt_init(m, sample_seed(loader_seed, epoch, id, FFCV_POLICY_OP));
  const double u0 = mt_double(m), u1 = mt_double(m), u2 = mt_double(m);
  const int op = min(FFCV_POLICY_NOPS - 1, (int)cj_mul(u0, (double)FFCV_POLICY_NOPS));
  const int bin = min(nbins - 1, (int)cj_mul(u1, (double)nbins));
  const bool neg = u2 < 0.5;
  const double v = table[op * nbins + bin];
  const double sv = neg && op >= POL_SHEAR_X && op <= POL_SHARPNESS ? -v : v;
  const double ratio = cj_add(1.0, sv);
  const uint64_t uk = (uint64_t)k, uB = (uint64_t)B;
  o.op[k] = (uint8_t)op;

  // colour programs: brightness, saturation, contrast | solarize
  const int cj_op[4] = {POL_BRIGHTNESS, POL_COLOR, POL_CONTRAST, POL_SOLARIZE};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool on = op == cj_op[i];
    o.cj_apply[i * uB + uk] = (uint8_t)on;
    o.cj_ratio[i * uB + uk] = i == 3 ? (on ? v : 256.0) : (on ? ratio : 1.0);
  }
  // tone program: posterize, autocontrast, equalize
  o.tone_apply[uk] = (uint8_t)(op == POL_POSTERIZE);
  o.tone_apply[uB + uk] = (uint8_t)(op == POL_AUTOCONTRAST);
  o.tone_apply[2 * uB + uk] = (uint8_t)(op == POL_EQUALIZE);
  o.tone_bits[k] = op == POL_POSTERIZE ? (uint8_t)(v < 1.0 ? 1.0 : (v > 8.0 ? 8.0 : v)) : (uint8_t)8;
  // affine: the one non-zero argument, scale 1
  o.aff_apply[k] = (uint8_t)(op >= POL_SHEAR_X && op <= POL_ROTATE);
  affine_matrix(op == POL_ROTATE ? sv : 0.0, op == POL_TRANSLATE_X ? sv : 0.0, op == POL_TRANSLATE_Y ? sv : 0.0, 1.0,
                op == POL_SHEAR_X ? sv : 0.0, op == POL_SHEAR_Y ? sv : 0.0, H, W, o.aff_coef + 6 * uk);
  // sharpness: every other image is left to the launches before it
  o.sharp_apply[k] = op == POL_SHARPNESS ? (uint8_t)1 : (uint8_t)2;
  o.sharp_factor[k] = op == POL_SHARPNESS ? (float)ratio : 1.0f;
  return m.err;
}

__global__ void __launch_bounds__(64) policy_draw_kernel(const uint64_t *__restrict__ ids, int B, uint64_t loader_seed,
                                                         uint64_t epoch, int nbins, const double *__restrict__ table,
                                                         int H, int W, PolicyOut o, int32_t *__restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int err = draw_policy(k, B, ids[k], loader_seed, epoch, nbins, table, H, W, o);
  if (status) status[k] = err ? FFCV_SAMPLE_RNG : FFCV_SAMPLE_OK;
}

static bool policy_args_ok(const char *who, const void *ids, int batch, int nbins, const void *table, int H, int W,
                           const PolicyOut &o) {
  if (batch < 0 || !ids || !table || !o.op || !o.cj_apply || !o.cj_ratio || !o.tone_apply || !o.tone_bits ||
      !o.aff_apply || !o.aff_coef || !o.sharp_apply || !o.sharp_factor || nbins < 2 || nbins > 256 || H <= 0 ||
      W <= 0 || H > FFCV_AFFINE_MAX_DIM || W > FFCV_AFFINE_MAX_DIM) {
    ffcv::set_error("%s: invalid arguments (batch %d, %d bins, %dx%d)", who, batch, nbins, H, W);
    return false;
  }
  return true;
}

// ---------------------------------------------------------- C ABI -------
extern "C" {

int ffcv_policy_draw_batch(void *stream, const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch,
                           int nbins, const double *table, int height, int width, uint8_t *op, uint8_t *cj_apply,
                           double *cj_ratio, uint8_t *tone_apply, uint8_t *tone_bits, uint8_t *aff_apply,
                           int64_t *aff_coef, uint8_t *sharp_apply, float *sharp_factor, int32_t *status) {
  const PolicyOut o = {op, cj_apply, cj_ratio, tone_apply, tone_bits, aff_apply, aff_coef, sharp_apply, sharp_factor};
  if (!policy_args_ok("ffcv_policy_draw_batch", sample_ids, batch, nbins, table, height, width, o)) return FFCV_EINVAL;
  return ffcv::launch_draw("policy_draw_kernel", policy_draw_kernel, stream, batch, sample_ids, batch, loader_seed,
                           epoch, nbins, table, height, width, o, status);
}

int ffcv_policy_draw_batch_host(const uint64_t *sample_ids, int batch, uint64_t loader_seed, uint64_t epoch, int nbins,
                                const double *table, int height, int width, uint8_t *op, uint8_t *cj_apply,
                                double *cj_ratio, uint8_t *tone_apply, uint8_t *tone_bits, uint8_t *aff_apply,
                                int64_t *aff_coef, uint8_t *sharp_apply, float *sharp_factor) {
  const PolicyOut o = {op, cj_apply, cj_ratio, tone_apply, tone_bits, aff_apply, aff_coef, sharp_apply, sharp_factor};
  if (!policy_args_ok("ffcv_policy_draw_batch_host", sample_ids, batch, nbins, table, height, width, o))
    return FFCV_EINVAL;
  return ffcv::host_draw("ffcv_policy_draw_batch_host", batch, [&](int k) {
    return draw_policy(k, batch, sample_ids[k], loader_seed, epoch, nbins, table, height, width, o);
  });
}

}  // extern "C"
