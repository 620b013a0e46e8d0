// inr_api_offgrid.hip -- the entries of the C-ABI (include/inr_abi.h) for the off-grid operators: inr_nudft, its conjugate
// transpose, the Kaiser-Bessel gridding form of both, and the coil product fused with that form for off-grid SENSE fits.
// Each checks null pointers, shapes, alignment, scratch size and
// overlaps, in that order, then launches and maps the hipError_t to a code; none allocates device memory or syncs.
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "inr_host.h"

static_assert(INR_NUDFT_TILE == inr::NUDFT_TILE, "inr_abi.h and inr_aux.h disagree");
static_assert(INR_NUFFT_TILE == inr::NUFFT_TILE && INR_NUFFT_TAPS == inr::NUFFT_TAPS, "inr_abi.h and inr_aux.h disagree");

// one operand of a call: `bytes` from p, p a multiple of `align`; p == nullptr: an optional operand that is absent
struct Span {
  const void* p;
  int64_t bytes;
  const char* name;
  unsigned align;
};
using Spans = std::initializer_list<Span>;

static int null_check(const char* who, std::initializer_list<const void*> required) {
  for (const void* p : required)
    if (p == nullptr) return fail(INR_ERR_INVALID, "%s: null argument", who);
  return INR_OK;
}

static int scratch_check(const char* who, const float* scratch, int64_t have, int64_t need) {
  if (((uintptr_t)scratch & 15u) != 0) return fail(INR_ERR_INVALID, "%s: scratch is not 16-byte aligned", who);
  if (have < need)
    return fail(INR_ERR_INVALID, "%s: scratch holds %lld floats, needs %lld", who, (long long)have, (long long)need);
  return INR_OK;
}

static int overlap_check(const char* who, const Span& a, const Span& b) {
  if (a.p != nullptr && b.p != nullptr && ranges_overlap(a.p, a.bytes, b.p, b.bytes))
    return fail(INR_ERR_INVALID, "%s: %s overlaps %s", who, a.name, b.name);
  return INR_OK;
}

// every operand aligned; the scratch aligned and of `need` floats; no output -- the scratch is one -- shares a byte with
// an input or with another output
static int operands_check(const char* who, Spans outs, Spans ins, const float* scratch, int64_t have, int64_t need) {
  for (Spans list : {outs, ins})
    for (const Span& s : list)
      if (((uintptr_t)s.p & (s.align - 1)) != 0)
        return fail(INR_ERR_INVALID, "%s: %s is not %u-byte aligned", who, s.name, s.align);
  if (int rc = scratch_check(who, scratch, have, need)) return rc;
  const Span scr = {scratch, need * 4, "scratch", 16};
  for (const Span& o : outs) {
    for (const Span& i : ins)
      if (int rc = overlap_check(who, o, i)) return rc;
    if (int rc = overlap_check(who, scr, o)) return rc;
  }
  for (const Span& i : ins)
    if (int rc = overlap_check(who, scr, i)) return rc;
  return INR_OK;
}

// ---- off-grid samples of the continuous k-space (inr_nudft.hip) ----
static int nudft_check(int32_t C, int64_t H, int64_t W, int64_t M, const char* who) {
  if (int rc = coil_count_check(C, "C", who)) return rc;
  if (H < 1 || W < 1 || H >= (1LL << 31) || W >= (1LL << 31) || H * W >= (1LL << 31))
    return fail(INR_ERR_INVALID, "%s: H = %lld, W = %lld (each >= 1, H * W < 2^31)", who, (long long)H, (long long)W);
  if (M < 1 || M >= (1LL << 31)) return fail(INR_ERR_INVALID, "%s: M = %lld (1 <= M < 2^31 samples per call)", who, (long long)M);
  return INR_OK;
}

// ---- ... and back onto the grid: the conjugate transpose (inr_nudft_adjoint.hip) ----
static int adjoint_nudft_check(int32_t C, int64_t H, int64_t W, int64_t M, const char* who) {
  if (int rc = nudft_check(C, H, W, M, who)) return rc;
  if (H > (1LL << 31) - 64 || W > (1LL << 31) - 64)  // the tables pad both axes to 64
    return fail(INR_ERR_INVALID, "%s: H = %lld, W = %lld (each <= 2^31 - 64)", who, (long long)H, (long long)W);
  return INR_OK;
}

// ---- the same two operators by Kaiser-Bessel gridding around the caller's FFT (inr_nufft.hip) ----
static int nufft_check(int32_t C, int64_t H, int64_t W, int64_t M, const char* who) {
  if (int rc = nudft_check(C, H, W, M, who)) return rc;
  if (H < INR_NUFFT_TAPS / 2 || W < INR_NUFFT_TAPS / 2)  // on 2 n < 6 cells two taps of a sample would share a cell
    return fail(INR_ERR_INVALID, "%s: H = %lld, W = %lld (each >= %d)", who, (long long)H, (long long)W, INR_NUFFT_TAPS / 2);
  return INR_OK;
}

// bin_start where the host can read it (pinned host memory): 0 = bin_start[0] <= ... <= bin_start[T] = M
static int nufft_bins_check(const char* who, const int32_t* bin_start, int64_t T, int64_t M) {
  hipPointerAttribute_t attr;
  memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, bin_start) != hipSuccess) {
    (void)hipGetLastError();  // a pointer the runtime does not know: nothing to check here
    return INR_OK;
  }
  if (attr.type != hipMemoryTypeHost || attr.hostPointer == nullptr) return INR_OK;
  const int32_t* b = static_cast<const int32_t*>(attr.hostPointer);
  bool ok = b[0] == 0 && b[T] == M;
  for (int64_t i = 0; ok && i < T; ++i) ok = b[i] <= b[i + 1];
  if (!ok)
    return fail(INR_ERR_INVALID, "%s: bin_start is not 0 = b[0] <= ... <= b[%lld] = %lld", who, (long long)T,
                (long long)M);
  return INR_OK;
}

// prepare and finish: the image [C][H][W][2], the grid [C][2H][2W][2], the two apodisation vectors
static int nufft_image_grid_check(const float* image, const float* grid, const float* apod_y, const float* apod_x, int32_t C,
                                  int64_t H, int64_t W, bool grid_is_output, const char* who) {
  if (image == nullptr || grid == nullptr || apod_y == nullptr || apod_x == nullptr)
    return fail(INR_ERR_INVALID, "%s: null argument", who);
  if (int rc = nufft_check(C, H, W, 1, who)) return rc;
  if (((uintptr_t)image & 7u) != 0) return fail(INR_ERR_INVALID, "%s: %s is not 8-byte aligned", who, grid_is_output ? "img" : "out");
  if (((uintptr_t)grid & 15u) != 0) return fail(INR_ERR_INVALID, "%s: grid is not 16-byte aligned", who);
  if ((((uintptr_t)apod_y | (uintptr_t)apod_x) & 3u) != 0)
    return fail(INR_ERR_INVALID, "%s: apod_y / apod_x is not 4-byte aligned", who);
  const int64_t image_bytes = (int64_t)C * H * W * 8, grid_bytes = 4 * image_bytes;
  const void* out = grid_is_output ? grid : image;
  const int64_t out_bytes = grid_is_output ? grid_bytes : image_bytes;
  if (ranges_overlap(grid, grid_bytes, image, image_bytes) || ranges_overlap(out, out_bytes, apod_y, H * 4) ||
      ranges_overlap(out, out_bytes, apod_x, W * 4))
    return fail(INR_ERR_INVALID, "%s: the output overlaps an input", who);
  return INR_OK;
}

extern "C" {

int inr_nudft_scratch(int32_t C, int64_t H, int64_t W, int64_t M, int64_t* scratch_floats) {
  if (scratch_floats == nullptr) return fail(INR_ERR_INVALID, "inr_nudft_scratch: null argument");
  if (int rc = nudft_check(C, H, W, M, "inr_nudft_scratch")) return rc;
  *scratch_floats = inr::nudft_scratch_floats(H, W, M);
  return INR_OK;
}

int inr_nudft(const float* img, int32_t C, int64_t H, int64_t W, const double* pos, int64_t M, float* out,
              float* scratch, int64_t scratch_floats, void* stream) {
  const char* who = "inr_nudft";
  if (int rc = null_check(who, {img, pos, out, scratch})) return rc;
  if (int rc = nudft_check(C, H, W, M, who)) return rc;
  if (int rc = operands_check(who, {{out, (int64_t)C * M * 8, "out", 8}},
                              {{img, (int64_t)C * H * W * 8, "img", 8}, {pos, M * 16, "pos", 8}}, scratch,
                              scratch_floats, inr::nudft_scratch_floats(H, W, M)))
    return rc;
  hipError_t e = inr::launch_nudft(img, C, (int)H, (int)W, pos, M, out, scratch, (hipStream_t)stream);
  return hip_done(e, who);
}

int inr_adjoint_nudft_scratch(int32_t C, int64_t H, int64_t W, int64_t M, int64_t* scratch_floats) {
  if (scratch_floats == nullptr) return fail(INR_ERR_INVALID, "inr_adjoint_nudft_scratch: null argument");
  if (int rc = adjoint_nudft_check(C, H, W, M, "inr_adjoint_nudft_scratch")) return rc;
  *scratch_floats = inr::adjoint_nudft_scratch_floats(H, W, M);
  return INR_OK;
}

int inr_adjoint_nudft(const float* val, const double* pos, const float* w, int32_t C, int64_t H, int64_t W, int64_t M,
                      float* out, float* scratch, int64_t scratch_floats, void* stream) {
  const char* who = "inr_adjoint_nudft";
  if (int rc = null_check(who, {val, pos, out, scratch})) return rc;
  if (int rc = adjoint_nudft_check(C, H, W, M, who)) return rc;
  if (int rc = operands_check(who, {{out, (int64_t)C * H * W * 8, "out", 8}},
                              {{val, (int64_t)C * M * 8, "val", 8}, {pos, M * 16, "pos", 8}, {w, M * 4, "w", 4}}, scratch,
                              scratch_floats, inr::adjoint_nudft_scratch_floats(H, W, M)))
    return rc;
  hipError_t e = inr::launch_adjoint_nudft(val, pos, w, C, (int)H, (int)W, M, out, scratch, (hipStream_t)stream);
  return hip_done(e, who);
}

int inr_nufft_scratch(int32_t C, int64_t H, int64_t W, int64_t M, int64_t* scratch_floats) {
  if (scratch_floats == nullptr) return fail(INR_ERR_INVALID, "inr_nufft_scratch: null argument");
  if (int rc = nufft_check(C, H, W, M, "inr_nufft_scratch")) return rc;
  *scratch_floats = inr::nufft_scratch_floats(M);
  return INR_OK;
}

int inr_nufft_prepare(const float* img, const float* apod_y, const float* apod_x, int32_t C, int64_t H, int64_t W,
                      float* grid, void* stream) {
  if (int rc = nufft_image_grid_check(img, grid, apod_y, apod_x, C, H, W, true, "inr_nufft_prepare")) return rc;
  hipError_t e = inr::launch_nufft_prepare(img, apod_y, apod_x, C, (int)H, (int)W, grid, (hipStream_t)stream);
  return hip_done(e, "inr_nufft_prepare");
}

int inr_nufft_finish(const float* grid, const float* apod_y, const float* apod_x, int32_t C, int64_t H, int64_t W,
                     float* out, void* stream) {
  if (int rc = nufft_image_grid_check(out, grid, apod_y, apod_x, C, H, W, false, "inr_nufft_finish")) return rc;
  hipError_t e = inr::launch_nufft_finish(grid, apod_y, apod_x, C, (int)H, (int)W, out, (hipStream_t)stream);
  return hip_done(e, "inr_nufft_finish");
}

static int nufft_interp(const char* who, bool plain, const float* grid, const double* pos, int32_t C, int64_t H, int64_t W,
                        int64_t M, float* out, float* scratch, int64_t scratch_floats, void* stream) {
  if (int rc = null_check(who, {grid, pos, out, scratch})) return rc;
  if (int rc = nufft_check(C, H, W, M, who)) return rc;
  if (int rc = operands_check(who, {{out, (int64_t)C * M * 8, "out", 8}},
                              {{grid, (int64_t)C * H * W * 32, "grid", 16}, {pos, M * 16, "pos", 8}}, scratch,
                              scratch_floats, inr::nufft_scratch_floats(M)))
    return rc;
  hipError_t e = inr::launch_nufft_interp(grid, pos, C, (int)H, (int)W, M, plain, out, scratch, (hipStream_t)stream);
  return hip_done(e, who);
}

static int nufft_spread(const char* who, bool plain, const float* val, const double* pos, const float* w,
                        const int32_t* bin_start, const int32_t* order, int32_t C, int64_t H, int64_t W, int64_t M,
                        float* grid, float* scratch, int64_t scratch_floats, void* stream) {
  if (int rc = null_check(who, {val, pos, bin_start, order, grid, scratch})) return rc;
  if (int rc = nufft_check(C, H, W, M, who)) return rc;
  const int64_t T = inr::nufft_bin_count(H, W);
  if (int rc = operands_check(who, {{grid, (int64_t)C * H * W * 32, "grid", 16}},
                              {{val, (int64_t)C * M * 8, "val", 8}, {pos, M * 16, "pos", 8}, {w, M * 4, "w", 4},
                               {bin_start, (T + 1) * 4, "bin_start", 4}, {order, M * 4, "order", 4}},
                              scratch, scratch_floats, inr::nufft_scratch_floats(M)))
    return rc;
  if (int rc = nufft_bins_check(who, bin_start, T, M)) return rc;
  hipError_t e = inr::launch_nufft_spread(val, pos, w, bin_start, order, C, (int)H, (int)W, M, plain, grid, scratch,
                                          (hipStream_t)stream);
  return hip_done(e, who);
}

int inr_nufft_interp(const float* grid, const double* pos, int32_t C, int64_t H, int64_t W, int64_t M, float* out,
                     float* scratch, int64_t scratch_floats, void* stream) {
  return nufft_interp("inr_nufft_interp", false, grid, pos, C, H, W, M, out, scratch, scratch_floats, stream);
}

int inr_nufft_interp_plain(const float* grid, const double* pos, int32_t C, int64_t H, int64_t W, int64_t M, float* out,
                           float* scratch, int64_t scratch_floats, void* stream) {
  return nufft_interp("inr_nufft_interp_plain", true, grid, pos, C, H, W, M, out, scratch, scratch_floats, stream);
}

int inr_nufft_spread(const float* val, const double* pos, const float* w, const int32_t* bin_start, const int32_t* order,
                     int32_t C, int64_t H, int64_t W, int64_t M, float* grid, float* scratch, int64_t scratch_floats,
                     void* stream) {
  return nufft_spread("inr_nufft_spread", false, val, pos, w, bin_start, order, C, H, W, M, grid, scratch, scratch_floats,
                      stream);
}

int inr_nufft_spread_plain(const float* val, const double* pos, const float* w, const int32_t* bin_start,
                           const int32_t* order, int32_t C, int64_t H, int64_t W, int64_t M, float* grid, float* scratch,
                           int64_t scratch_floats, void* stream) {
  return nufft_spread("inr_nufft_spread_plain", true, val, pos, w, bin_start, order, C, H, W, M, grid, scratch,
                      scratch_floats, stream);
}

// ---- the coil product fused with prepare / finish on the plain-layout grid (inr_sense_nufft.hip) ----
// img or dimg [H*W,2], maps [G,H*W,2], grid [G,2H,2W,2], the two apodisation vectors; `image_is_output`: finish
static int sense_nufft_check(const char* who, const float* image, const char* image_name, const float* maps,
                             const float* grid, const float* apod_y, const float* apod_x, int32_t G, int64_t H, int64_t W,
                             float scale, bool image_is_output) {
  if (int rc = null_check(who, {image, maps, grid, apod_y, apod_x})) return rc;
  if (int rc = nufft_check(G, H, W, 1, who)) return rc;
  if (!std::isfinite(scale)) return fail(INR_ERR_INVALID, "%s: scale = %g (must be finite)", who, (double)scale);
  const int64_t plane = H * W * 8;
  const Span im = {image, plane, image_name, 8}, mp = {maps, G * plane, "maps", 8}, gr = {grid, 4 * G * plane, "grid", 8};
  const Span ay = {apod_y, H * 4, "apod_y", 4}, ax = {apod_x, W * 4, "apod_x", 4};
  for (const Span& s : {im, mp, gr, ay, ax})
    if (((uintptr_t)s.p & (s.align - 1)) != 0) return fail(INR_ERR_INVALID, "%s: %s is not %u-byte aligned", who, s.name, s.align);
  const Span& out = image_is_output ? im : gr;
  for (const Span& in : {image_is_output ? gr : im, mp, ay, ax})
    if (int rc = overlap_check(who, out, in)) return rc;
  return INR_OK;
}

int inr_sense_nufft_prepare(const float* img, const float* maps, const float* apod_y, const float* apod_x, int32_t G,
                            int64_t H, int64_t W, float scale, float* grid, void* stream) {
  const char* who = "inr_sense_nufft_prepare";
  if (int rc = sense_nufft_check(who, img, "img", maps, grid, apod_y, apod_x, G, H, W, scale, false)) return rc;
  hipError_t e = inr::launch_sense_nufft_prepare(img, maps, apod_y, apod_x, G, (int)H, (int)W, scale, grid,
                                                 (hipStream_t)stream);
  return hip_done(e, who);
}

int inr_sense_nufft_finish(const float* grid, const float* maps, const float* apod_y, const float* apod_x, int32_t G,
                           int64_t H, int64_t W, float scale, float* dimg, int32_t accumulate, void* stream) {
  const char* who = "inr_sense_nufft_finish";
  if (int rc = sense_nufft_check(who, dimg, "dimg", maps, grid, apod_y, apod_x, G, H, W, scale, true)) return rc;
  if (accumulate != 0 && accumulate != 1) return fail(INR_ERR_INVALID, "%s: accumulate = %d (0 or 1)", who, (int)accumulate);
  hipError_t e = inr::launch_sense_nufft_finish(grid, maps, apod_y, apod_x, G, (int)H, (int)W, scale, dimg, accumulate != 0,
                                                (hipStream_t)stream);
  return hip_done(e, who);
}

}  // extern "C"
