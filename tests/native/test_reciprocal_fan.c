/* spfft_amd_multi_transform_reciprocal_fan_out / fan_in and their float twins
 * through the C API: three transforms (one and two clones) on a sparse 6x5x4
 * index set with one kernel per member, on two consecutive calls, against single
 * spfft_amd_transform_apply_reciprocal calls (which tests/native/
 * test_reciprocal.c checks against direct sums): fan-out member i against
 * apply_reciprocal with K_i on the same input, its values output against the
 * single call's, fan-in against the sum of the members' single results (the
 * operator is linear), with real and with complex kernels and both scalings. A
 * repeated grid, null arrays, a null entry, a bad scaling, unequal transforms
 * and a null handle must be errors and leave the transforms usable; n = 0 is a
 * no-op, n = 1 the single call. Runs on the host engine and, when a device is
 * visible, on the GPU (host pointers, host space domains). */
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
#define DEFINE_RUN(NAME, REAL, GRID, TRANSFORM, GRID_CREATE, GRID_DESTROY, CREATE, CLONE, DESTROY, SPACE,  \
                   SINGLE, FAN_OUT, FAN_IN, QUERY, TOL)                                                    \
  static REAL NAME##_f[NT][2 * NS], NAME##_kern[NT][2 * NS], NAME##_ref[NT][2 * NS], NAME##_sum[2 * NS],   \
      NAME##_vals[2 * NS], NAME##_vref[2 * NS];                                                            \
  static double NAME##_err(const REAL* got, const REAL* want, int count) {                                 \
    double num = 0, den = 0;                                                                               \
    for (int i = 0; i < count; ++i) {                                                                      \
      num = fmax(num, fabs((double)got[i] - (double)want[i]));                                             \
      den = fmax(den, fabs((double)want[i]));                                                              \
    }                                                                                                      \
    return den > 0 ? num / den : 1.0;                                                                      \
  }                                                                                                        \
  static void NAME(SpfftProcessingUnitType pu) {                                                           \
    const char* where = pu == SPFFT_PU_GPU ? "gpu" : "host";                                               \
    const SpfftProcessingUnitType loc = SPFFT_PU_HOST;                                                     \
    const int nv = make_indices();                                                                         \
    for (int t = 0; t < NT; ++t) {                                                                         \
      for (int i = 0; i < NS; ++i) {                                                                       \
        NAME##_f[t][2 * i] = (REAL)(1.0 + 0.125 * ((i + 3 * t) % 11) - 0.01 * i);                          \
        NAME##_f[t][2 * i + 1] = (REAL)(0.5 - 0.25 * ((i + t) % 7));                                       \
      }                                                                                                    \
      for (int k = 0; k < nv; ++k) {                                                                       \
        NAME##_kern[t][2 * k] = (REAL)(0.5 + 0.0625 * ((k + t) % 5));                                      \
        NAME##_kern[t][2 * k + 1] = (REAL)(0.25 - 0.125 * ((k + 2 * t) % 3));                              \
      }                                                                                                    \
    }                                                                                                      \
    GRID grid = NULL, grid2 = NULL;                                                                        \
    TRANSFORM ts[NT] = {NULL, NULL, NULL};                                                                 \
    TRANSFORM other = NULL;                                                                                \
    CHECK(GRID_CREATE(&grid, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);                               \
    CHECK(CREATE(&ts[0], grid, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv, SPFFT_INDEX_TRIPLETS, indices) ==  \
          SPFFT_SUCCESS);                                                                                  \
    GRID_DESTROY(grid);                                                                                    \
    /* the same dimensions, fewer values */                                                                \
    CHECK(GRID_CREATE(&grid2, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);                              \
    CHECK(CREATE(&other, grid2, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv - NZ, SPFFT_INDEX_TRIPLETS,        \
                 indices) == SPFFT_SUCCESS);                                                               \
    GRID_DESTROY(grid2);                                                                                   \
    if (!ts[0] || !other) return;                                                                          \
    CHECK(CLONE(ts[0], &ts[1]) == SPFFT_SUCCESS);                                                          \
    CHECK(CLONE(ts[0], &ts[2]) == SPFFT_SUCCESS);                                                          \
    if (!ts[1] || !ts[2]) return;                                                                          \
    REAL* space[NT] = {NULL, NULL, NULL};                                                                  \
    for (int t = 0; t < NT; ++t) CHECK(SPACE(ts[t], loc, &space[t]) == SPFFT_SUCCESS);                     \
    if (!space[0] || !space[1] || !space[2]) return;                                                       \
    const REAL* ks[NT] = {NAME##_kern[0], NAME##_kern[1], NAME##_kern[2]};                                 \
    const REAL* hole[NT] = {NAME##_kern[0], NULL, NAME##_kern[2]};                                         \
    TRANSFORM twice[NT] = {ts[0], ts[1], ts[0]};                                                           \
    TRANSFORM gap[NT] = {ts[0], NULL, ts[2]};                                                              \
    TRANSFORM odd[NT] = {ts[0], other, ts[2]};                                                             \
    const SpfftScalingType none = SPFFT_NO_SCALING, bad = (SpfftScalingType)7;                             \
    CHECK(FAN_OUT(NT, twice, loc, ks, 1, NULL, none) == SPFFT_INVALID_PARAMETER_ERROR);                    \
    CHECK(FAN_OUT(NT, gap, loc, ks, 1, NULL, none) == SPFFT_INVALID_HANDLE_ERROR);                         \
    CHECK(FAN_OUT(NT, odd, loc, ks, 1, NULL, none) == SPFFT_INVALID_PARAMETER_ERROR);                      \
    CHECK(FAN_OUT(NT, NULL, loc, ks, 1, NULL, none) == SPFFT_INVALID_PARAMETER_ERROR);                     \
    CHECK(FAN_OUT(NT, ts, loc, NULL, 1, NULL, none) == SPFFT_INVALID_PARAMETER_ERROR);                     \
    CHECK(FAN_OUT(NT, ts, loc, hole, 1, NULL, none) == SPFFT_INVALID_PARAMETER_ERROR);                     \
    CHECK(FAN_OUT(NT, ts, loc, ks, 1, NULL, bad) == SPFFT_INVALID_PARAMETER_ERROR);                        \
    CHECK(FAN_OUT(0, NULL, loc, NULL, 0, NULL, none) == SPFFT_SUCCESS);                                    \
    CHECK(FAN_IN(NT, twice, loc, ks, 1, none) == SPFFT_INVALID_PARAMETER_ERROR);                           \
    CHECK(FAN_IN(NT, gap, loc, ks, 1, none) == SPFFT_INVALID_HANDLE_ERROR);                                \
    CHECK(FAN_IN(NT, odd, loc, ks, 1, none) == SPFFT_INVALID_PARAMETER_ERROR);                             \
    CHECK(FAN_IN(NT, NULL, loc, ks, 1, none) == SPFFT_INVALID_PARAMETER_ERROR);                            \
    CHECK(FAN_IN(NT, ts, loc, NULL, 1, none) == SPFFT_INVALID_PARAMETER_ERROR);                            \
    CHECK(FAN_IN(NT, ts, loc, hole, 1, none) == SPFFT_INVALID_PARAMETER_ERROR);                            \
    CHECK(FAN_IN(NT, ts, loc, ks, 1, bad) == SPFFT_INVALID_PARAMETER_ERROR);                               \
    CHECK(FAN_IN(0, NULL, loc, NULL, 0, none) == SPFFT_SUCCESS);                                           \
    int fused = -1;                                                                                        \
    CHECK(QUERY(ts[0], NT, &fused) == SPFFT_SUCCESS && (fused == 0 || fused == 1));                        \
    CHECK(pu == SPFFT_PU_GPU || fused == 0);                                                               \
    CHECK(QUERY(ts[0], NT, NULL) == SPFFT_INVALID_PARAMETER_ERROR);                                        \
    CHECK(QUERY(NULL, NT, &fused) == SPFFT_INVALID_HANDLE_ERROR);                                          \
    for (int c = 0; c < 2; ++c)                                                                            \
      for (int s = 0; s < 2; ++s) {                                                                        \
        const SpfftScalingType scaling = s ? SPFFT_FULL_SCALING : SPFFT_NO_SCALING;                        \
        /* fan-out: member t against apply_reciprocal(K_t) on the input of member 0 */                     \
        for (int t = 0; t < NT; ++t) {                                                                     \
          for (int i = 0; i < 2 * NS; ++i) space[t][i] = NAME##_f[0][i];                                   \
          CHECK(SINGLE(ts[t], loc, ks[t], c, NAME##_vref, scaling) == SPFFT_SUCCESS);                      \
          for (int i = 0; i < 2 * NS; ++i) NAME##_ref[t][i] = space[t][i];                                 \
        }                                                                                                  \
        for (int rep = 0; rep < 2; ++rep) {                                                                \
          for (int i = 0; i < 2 * NS; ++i) space[0][i] = NAME##_f[0][i];                                   \
          for (int i = 0; i < 2 * nv; ++i) NAME##_vals[i] = (REAL)-1;                                      \
          CHECK(FAN_OUT(NT, ts, loc, ks, c, NAME##_vals, scaling) == SPFFT_SUCCESS);                       \
          double err = NAME##_err(NAME##_vals, NAME##_vref, 2 * nv);                                       \
          for (int t = 0; t < NT; ++t) err = fmax(err, NAME##_err(space[t], NAME##_ref[t], 2 * NS));       \
          printf("reciprocal_fan_out %s %s complex %d scaling %d rep %d: max rel error %.3e\n", #REAL,     \
                 where, c, s, rep, err);                                                                   \
          CHECK(err < TOL);                                                                                \
        }                                                                                                  \
        /* n = 1: the single call */                                                                       \
        for (int i = 0; i < 2 * NS; ++i) space[0][i] = NAME##_f[0][i];                                     \
        CHECK(FAN_OUT(1, ts, loc, ks, c, NULL, scaling) == SPFFT_SUCCESS);                                 \
        for (int i = 0; i < 2 * NS; ++i) CHECK(space[0][i] == NAME##_ref[0][i]);                           \
        /* fan-in: the sum of the members' single results */                                               \
        for (int i = 0; i < 2 * NS; ++i) NAME##_sum[i] = 0;                                                \
        for (int t = 0; t < NT; ++t) {                                                                     \
          for (int i = 0; i < 2 * NS; ++i) space[t][i] = NAME##_f[t][i];                                   \
          CHECK(SINGLE(ts[t], loc, ks[t], c, NULL, scaling) == SPFFT_SUCCESS);                             \
          for (int i = 0; i < 2 * NS; ++i) NAME##_sum[i] += space[t][i];                                   \
        }                                                                                                  \
        for (int rep = 0; rep < 2; ++rep) {                                                                \
          for (int t = 0; t < NT; ++t)                                                                     \
            for (int i = 0; i < 2 * NS; ++i) space[t][i] = NAME##_f[t][i];                                 \
          CHECK(FAN_IN(NT, ts, loc, ks, c, scaling) == SPFFT_SUCCESS);                                     \
          const double err = NAME##_err(space[0], NAME##_sum, 2 * NS);                                     \
          printf("reciprocal_fan_in %s %s complex %d scaling %d rep %d: max rel error %.3e\n", #REAL,      \
                 where, c, s, rep, err);                                                                   \
          CHECK(err < TOL);                                                                                \
          for (int t = 1; t < NT; ++t)                                                                     \
            for (int i = 0; i < 2 * NS; ++i) CHECK(space[t][i] == NAME##_f[t][i]);                         \
        }                                                                                                  \
      }                                                                                                    \
    for (int t = 0; t < NT; ++t) DESTROY(ts[t]);                                                           \
    DESTROY(other);                                                                                        \
  }

DEFINE_RUN(run_double, double, SpfftGrid, SpfftTransform, spfft_grid_create, spfft_grid_destroy,
           spfft_transform_create, spfft_transform_clone, spfft_transform_destroy,
           spfft_transform_get_space_domain, spfft_amd_transform_apply_reciprocal,
           spfft_amd_multi_transform_reciprocal_fan_out, spfft_amd_multi_transform_reciprocal_fan_in,
           spfft_amd_transform_reciprocal_fan_fused, 1e-12)
DEFINE_RUN(run_float, float, SpfftFloatGrid, SpfftFloatTransform, spfft_float_grid_create,
           spfft_float_grid_destroy, spfft_float_transform_create, spfft_float_transform_clone,
           spfft_float_transform_destroy, spfft_float_transform_get_space_domain,
           spfft_amd_float_transform_apply_reciprocal, spfft_amd_float_multi_transform_reciprocal_fan_out,
           spfft_amd_float_multi_transform_reciprocal_fan_in, spfft_amd_float_transform_reciprocal_fan_fused,
           2e-5)

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
