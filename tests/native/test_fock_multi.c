/* spfft_amd_multi_transform_accumulate_fock and its float twin through the C
 * API: three transforms (one and two clones) on a sparse 6x5x4 index set, one a
 * per transform, a shared b and kernel, weights of both signs, into one acc on
 * two consecutive calls, against the same pairs as single
 * spfft_amd_transform_accumulate_fock calls (which tests/native/test_fock.c
 * checks against direct sums), with a real and with a complex kernel and both
 * scalings. A repeated grid, null arrays, a null entry, a bad scaling and a
 * null handle must be errors and leave the transforms usable; n = 0 is a
 * no-op. Runs on the host engine and, when a device is visible, on the GPU
 * (host pointers). */
#include <math.h>
#include <stdio.h>

#include "spfft/amd.h"
#include "spfft/spfft.h"

#define NX 6
#define NY 5
#define NZ 4
#define NS (NX * NY * NZ)
#define NT 3

static int failed = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL line %d: %s\n", __LINE__, #cond);              \
      ++failed;                                                   \
    }                                                             \
  } while (0)

static int indices[3 * NS];

static int make_indices(void) {
  int nv = 0;
  for (int x = 0; x < NX; ++x)
    for (int y = 0; y < NY; ++y)
      for (int z = 0; z < NZ; ++z) {
        if ((x + 2 * y) % 4 == 3) continue; /* whole sticks left out */
        indices[3 * nv] = x;
        indices[3 * nv + 1] = y;
        indices[3 * nv + 2] = z;
        ++nv;
      }
  return nv;
}

/* one body per precision: REAL, the handle types and the entry points */
#define DEFINE_RUN(NAME, REAL, GRID, TRANSFORM, GRID_CREATE, GRID_DESTROY, CREATE, CLONE, DESTROY, SINGLE, \
                   MULTI, TOL)                                                                             \
  static REAL NAME##_a[NT][2 * NS], NAME##_b[2 * NS], NAME##_kern[2 * NS], NAME##_acc[2 * NS],             \
      NAME##_ref[2 * NS], NAME##_acc0[2 * NS];                                                             \
  static void NAME(SpfftProcessingUnitType pu) {                                                           \
    const char* where = pu == SPFFT_PU_GPU ? "gpu" : "host";                                               \
    const REAL w[NT] = {(REAL)-0.75, (REAL)0.5, (REAL)-1.25};                                              \
    const int nv = make_indices();                                                                         \
    for (int i = 0; i < NS; ++i) {                                                                         \
      for (int t = 0; t < NT; ++t) {                                                                       \
        NAME##_a[t][2 * i] = (REAL)(1.0 + 0.125 * ((i + 3 * t) % 11) - 0.01 * i);                          \
        NAME##_a[t][2 * i + 1] = (REAL)(0.5 - 0.25 * ((i + t) % 7));                                       \
      }                                                                                                    \
      NAME##_b[2 * i] = (REAL)(-0.75 + 0.25 * (i % 5));                                                    \
      NAME##_b[2 * i + 1] = (REAL)(0.125 * (i % 13) - 0.5);                                                \
      NAME##_acc0[2 * i] = (REAL)(0.5 - 0.0625 * (i % 17));                                                \
      NAME##_acc0[2 * i + 1] = (REAL)(0.25 * (i % 3) - 0.25);                                              \
    }                                                                                                      \
    for (int k = 0; k < nv; ++k) {                                                                         \
      NAME##_kern[2 * k] = (REAL)(0.5 + 0.0625 * (k % 5));                                                 \
      NAME##_kern[2 * k + 1] = (REAL)(0.25 - 0.125 * (k % 3));                                             \
    }                                                                                                      \
    GRID grid = NULL;                                                                                      \
    TRANSFORM ts[NT] = {NULL, NULL, NULL};                                                                 \
    CHECK(GRID_CREATE(&grid, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);                               \
    CHECK(CREATE(&ts[0], grid, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv, SPFFT_INDEX_TRIPLETS, indices) ==  \
          SPFFT_SUCCESS);                                                                                  \
    GRID_DESTROY(grid);                                                                                    \
    if (!ts[0]) return;                                                                                    \
    CHECK(CLONE(ts[0], &ts[1]) == SPFFT_SUCCESS);                                                          \
    CHECK(CLONE(ts[0], &ts[2]) == SPFFT_SUCCESS);                                                          \
    if (!ts[1] || !ts[2]) return;                                                                          \
    const REAL* as[NT] = {NAME##_a[0], NAME##_a[1], NAME##_a[2]};                                          \
    const REAL* bs[NT] = {NAME##_b, NAME##_b, NAME##_b};                                                   \
    const REAL* ks[NT] = {NAME##_kern, NAME##_kern, NAME##_kern};                                          \
    const REAL* hole[NT] = {NAME##_kern, NULL, NAME##_kern};                                               \
    TRANSFORM twice[NT] = {ts[0], ts[1], ts[0]};                                                           \
    TRANSFORM gap[NT] = {ts[0], NULL, ts[2]};                                                              \
    REAL* acc = NAME##_acc;                                                                                \
    for (int i = 0; i < 2 * NS; ++i) acc[i] = NAME##_acc0[i];                                              \
    CHECK(MULTI(NT, twice, as, bs, ks, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);     \
    CHECK(MULTI(NT, gap, as, bs, ks, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_HANDLE_ERROR);          \
    CHECK(MULTI(NT, NULL, as, bs, ks, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);      \
    CHECK(MULTI(NT, ts, NULL, bs, ks, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);      \
    CHECK(MULTI(NT, ts, as, NULL, ks, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);      \
    CHECK(MULTI(NT, ts, as, bs, NULL, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);      \
    CHECK(MULTI(NT, ts, as, bs, ks, 0, NULL, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);     \
    CHECK(MULTI(NT, ts, as, bs, ks, 0, w, NULL, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);       \
    CHECK(MULTI(NT, ts, as, bs, hole, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);      \
    CHECK(MULTI(NT, ts, hole, bs, ks, 0, w, acc, SPFFT_NO_SCALING) == SPFFT_INVALID_PARAMETER_ERROR);      \
    CHECK(MULTI(NT, ts, as, bs, ks, 0, w, acc, (SpfftScalingType)7) == SPFFT_INVALID_PARAMETER_ERROR);     \
    CHECK(MULTI(0, NULL, NULL, NULL, NULL, 0, NULL, NULL, SPFFT_NO_SCALING) == SPFFT_SUCCESS);             \
    for (int i = 0; i < 2 * NS; ++i) CHECK(acc[i] == NAME##_acc0[i]);                                      \
    for (int c = 0; c < 2; ++c)                                                                            \
      for (int s = 0; s < 2; ++s) {                                                                        \
        const SpfftScalingType scaling = s ? SPFFT_FULL_SCALING : SPFFT_NO_SCALING;                        \
        for (int i = 0; i < 2 * NS; ++i) acc[i] = NAME##_ref[i] = NAME##_acc0[i];                          \
        for (int rep = 0; rep < 2; ++rep) {                                                                \
          for (int t = 0; t < NT; ++t)                                                                     \
            CHECK(SINGLE(ts[t], as[t], bs[t], ks[t], c, w[t], NAME##_ref, NULL, scaling) == SPFFT_SUCCESS); \
          CHECK(MULTI(NT, ts, as, bs, ks, c, w, acc, scaling) == SPFFT_SUCCESS);                           \
          double num = 0, den = 0, upd = 0, updDen = 0;                                                    \
          for (int i = 0; i < 2 * NS; ++i) {                                                               \
            num = fmax(num, fabs((double)acc[i] - (double)NAME##_ref[i]));                                 \
            den = fmax(den, fabs((double)NAME##_ref[i]));                                                  \
            upd = fmax(upd, fabs(((double)acc[i] - NAME##_acc0[i]) - ((double)NAME##_ref[i] - NAME##_acc0[i]))); \
            updDen = fmax(updDen, fabs((double)NAME##_ref[i] - NAME##_acc0[i]));                           \
          }                                                                                                \
          printf("multi_accumulate_fock %s %s complex %d scaling %d rep %d: max rel error acc %.3e update %.3e\n", \
                 #REAL, where, c, s, rep, num / den, upd / updDen);                                        \
          CHECK(updDen > 0 && num / den < TOL && upd / updDen < TOL);                                      \
        }                                                                                                  \
      }                                                                                                    \
    for (int t = 0; t < NT; ++t) DESTROY(ts[t]);                                                           \
  }

DEFINE_RUN(run_double, double, SpfftGrid, SpfftTransform, spfft_grid_create, spfft_grid_destroy,
           spfft_transform_create, spfft_transform_clone, spfft_transform_destroy,
           spfft_amd_transform_accumulate_fock, spfft_amd_multi_transform_accumulate_fock, 1e-12)
DEFINE_RUN(run_float, float, SpfftFloatGrid, SpfftFloatTransform, spfft_float_grid_create,
           spfft_float_grid_destroy, spfft_float_transform_create, spfft_float_transform_clone,
           spfft_float_transform_destroy, spfft_amd_float_transform_accumulate_fock,
           spfft_amd_float_multi_transform_accumulate_fock, 2e-5)

int main(void) {
  run_double(SPFFT_PU_HOST);
  run_float(SPFFT_PU_HOST);
  if (spfft_amd_device_count() > 0) {
    run_double(SPFFT_PU_GPU);
    run_float(SPFFT_PU_GPU);
  } else {
    printf("SKIP gpu (no device)\n");
  }
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
