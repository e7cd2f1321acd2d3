/* spfft_amd_multi_transform_accumulate_density_fan / apply_local_fan and their
 * float twins through the C API: three transforms (one and two clones) on a
 * sparse 6x5x4 index set with one kernel per member and side, on two consecutive
 * calls, against single spfft_amd_transform_accumulate_density / apply_local
 * calls on premultiplied values (which tests/native/test_density.c and
 * test_apply_local.c check against direct sums), combined here in list order;
 * with real kernels and with complex kernels that have null (identity) entries
 * and, for the operator, both scalings and input == output. A repeated grid,
 * null arrays, a null input, output, density or potential, a bad scaling,
 * unequal transforms and a null handle must be errors and leave the transforms
 * usable; n = 0 is a no-op, n = 1 with null kernels the single call. Runs on the
 * host engine and, when a device is visible, on the GPU with host pointers. */
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
#define DEFINE_RUN(NAME, REAL, GRID, TRANSFORM, GRID_CREATE, GRID_DESTROY, CREATE, CLONE, DESTROY,         \
                   APPLY, DENSITY, DENSITY_FAN, APPLY_FAN, QUERY, TOL)                                     \
  static REAL NAME##_vals[2 * NS], NAME##_kern[NT][2 * NS], NAME##_pot[NT][NS], NAME##_pre[2 * NS],        \
      NAME##_res[2 * NS], NAME##_ref[2 * NS], NAME##_out[2 * NS], NAME##_rho[NS], NAME##_rhoref[NS];       \
  static double NAME##_err(const REAL* got, const REAL* want, int count) {                                 \
    double num = 0, den = 0;                                                                               \
    for (int i = 0; i < count; ++i) {                                                                      \
      num = fmax(num, fabs((double)got[i] - (double)want[i]));                                             \
      den = fmax(den, fabs((double)want[i]));                                                              \
    }                                                                                                      \
    return den > 0 ? num / den : 1.0;                                                                      \
  }                                                                                                        \
  /* out = in * K (add: out += in * K) over nv values; K null: the identity */                             \
  static void NAME##_mul(REAL* out, const REAL* in, const REAL* k, int cplx, int nv, int add) {            \
    for (int i = 0; i < nv; ++i) {                                                                         \
      const REAL re = in[2 * i], im = in[2 * i + 1];                                                       \
      REAL pr = re, pi = im;                                                                               \
      if (k && cplx) {                                                                                     \
        pr = re * k[2 * i] - im * k[2 * i + 1];                                                            \
        pi = re * k[2 * i + 1] + im * k[2 * i];                                                            \
      } else if (k) {                                                                                      \
        pr = re * k[i];                                                                                    \
        pi = im * k[i];                                                                                    \
      }                                                                                                    \
      out[2 * i] = add ? out[2 * i] + pr : pr;                                                             \
      out[2 * i + 1] = add ? out[2 * i + 1] + pi : pi;                                                     \
    }                                                                                                      \
  }                                                                                                        \
  static void NAME(SpfftProcessingUnitType pu) {                                                           \
    const char* where = pu == SPFFT_PU_GPU ? "gpu" : "host";                                               \
    const int nv = make_indices();                                                                         \
    for (int k = 0; k < nv; ++k) {                                                                         \
      NAME##_vals[2 * k] = (REAL)(1.0 + 0.125 * (k % 11) - 0.01 * k);                                      \
      NAME##_vals[2 * k + 1] = (REAL)(0.5 - 0.25 * (k % 7));                                               \
    }                                                                                                      \
    for (int t = 0; t < NT; ++t) {                                                                         \
      for (int k = 0; k < nv; ++k) {                                                                       \
        NAME##_kern[t][2 * k] = (REAL)(0.5 + 0.0625 * ((k + t) % 5));                                      \
        NAME##_kern[t][2 * k + 1] = (REAL)(0.25 - 0.125 * ((k + 2 * t) % 3));                              \
      }                                                                                                    \
      for (int i = 0; i < NS; ++i) NAME##_pot[t][i] = (REAL)(-1.0 + 0.125 * ((i + 5 * t) % 17));           \
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
    const REAL* ks[NT] = {NAME##_kern[0], NAME##_kern[1], NAME##_kern[2]};                                 \
    const REAL* ls[NT] = {NAME##_kern[2], NAME##_kern[0], NAME##_kern[1]};                                 \
    const REAL* ksn[NT] = {NULL, NAME##_kern[1], NAME##_kern[2]};                                          \
    const REAL* lsn[NT] = {NULL, NAME##_kern[2], NULL};                                                    \
    const REAL* none3[NT] = {NULL, NULL, NULL};                                                            \
    const REAL* vs[NT] = {NAME##_pot[0], NAME##_pot[1], NAME##_pot[2]};                                    \
    const REAL* vhole[NT] = {NAME##_pot[0], NULL, NAME##_pot[2]};                                          \
    const REAL ws[NT] = {(REAL)1.0, (REAL)0.5, (REAL)0.25};                                                \
    TRANSFORM twice[NT] = {ts[0], ts[1], ts[0]};                                                           \
    TRANSFORM gap[NT] = {ts[0], NULL, ts[2]};                                                              \
    TRANSFORM odd[NT] = {ts[0], other, ts[2]};                                                             \
    const SpfftScalingType none = SPFFT_NO_SCALING, bad = (SpfftScalingType)7;                             \
    const SpfftError inv = SPFFT_INVALID_PARAMETER_ERROR;                                                  \
    REAL* v = NAME##_vals;                                                                                 \
    REAL* o = NAME##_out;                                                                                  \
    REAL* r = NAME##_rho;                                                                                  \
    for (int i = 0; i < NS; ++i) r[i] = (REAL)0.5;                                                         \
    CHECK(DENSITY_FAN(NT, twice, v, ks, 1, ws, r) == inv);                                                 \
    CHECK(DENSITY_FAN(NT, gap, v, ks, 1, ws, r) == SPFFT_INVALID_HANDLE_ERROR);                            \
    CHECK(DENSITY_FAN(NT, odd, v, ks, 1, ws, r) == inv);                                                   \
    CHECK(DENSITY_FAN(NT, NULL, v, ks, 1, ws, r) == inv);                                                  \
    CHECK(DENSITY_FAN(NT, ts, v, NULL, 1, ws, r) == inv);                                                  \
    CHECK(DENSITY_FAN(NT, ts, v, ks, 1, NULL, r) == inv);                                                  \
    CHECK(DENSITY_FAN(NT, ts, NULL, ks, 1, ws, r) == inv);                                                 \
    CHECK(DENSITY_FAN(NT, ts, v, ks, 1, ws, NULL) == inv);                                                 \
    CHECK(DENSITY_FAN(0, NULL, NULL, NULL, 0, NULL, NULL) == SPFFT_SUCCESS);                               \
    for (int i = 0; i < NS; ++i) CHECK(r[i] == (REAL)0.5); /* no failed call touched rho */                \
    CHECK(APPLY_FAN(NT, twice, v, ks, vs, ls, 1, o, none) == inv);                                         \
    CHECK(APPLY_FAN(NT, gap, v, ks, vs, ls, 1, o, none) == SPFFT_INVALID_HANDLE_ERROR);                    \
    CHECK(APPLY_FAN(NT, odd, v, ks, vs, ls, 1, o, none) == inv);                                           \
    CHECK(APPLY_FAN(NT, NULL, v, ks, vs, ls, 1, o, none) == inv);                                          \
    CHECK(APPLY_FAN(NT, ts, v, NULL, vs, ls, 1, o, none) == inv);                                          \
    CHECK(APPLY_FAN(NT, ts, v, ks, NULL, ls, 1, o, none) == inv);                                          \
    CHECK(APPLY_FAN(NT, ts, v, ks, vs, NULL, 1, o, none) == inv);                                          \
    CHECK(APPLY_FAN(NT, ts, NULL, ks, vs, ls, 1, o, none) == inv);                                         \
    CHECK(APPLY_FAN(NT, ts, v, ks, vs, ls, 1, NULL, none) == inv);                                         \
    CHECK(APPLY_FAN(NT, ts, v, ks, vhole, ls, 1, o, none) == inv);                                         \
    CHECK(APPLY_FAN(NT, ts, v, ks, vs, ls, 1, o, bad) == inv);                                             \
    CHECK(APPLY_FAN(0, NULL, NULL, NULL, NULL, NULL, 0, NULL, none) == SPFFT_SUCCESS);                     \
    int fused = -1;                                                                                        \
    CHECK(QUERY(ts[0], NT, &fused) == SPFFT_SUCCESS && (fused == 0 || fused == 1));                        \
    CHECK(pu == SPFFT_PU_GPU || fused == 0);                                                               \
    CHECK(QUERY(ts[0], NT, NULL) == SPFFT_INVALID_PARAMETER_ERROR);                                        \
    CHECK(QUERY(NULL, NT, &fused) == SPFFT_INVALID_HANDLE_ERROR);                                          \
    /* real kernels everywhere, then complex kernels with null (identity) entries */                      \
    for (int c = 0; c < 2; ++c)                                                                            \
      for (int nul = c; nul <= c; ++nul) {                                                                 \
        const REAL* const* kin = nul ? ksn : ks;                                                           \
        const REAL* const* kout = nul ? lsn : ls;                                                          \
        /* density fan: single calls on premultiplied values, in list order */                             \
        for (int i = 0; i < NS; ++i) NAME##_rhoref[i] = (REAL)(0.125 * (i % 5));                           \
        for (int t = 0; t < NT; ++t) {                                                                     \
          NAME##_mul(NAME##_pre, v, kin[t], c, nv, 0);                                                     \
          CHECK(DENSITY(ts[t], NAME##_pre, ws[t], NAME##_rhoref) == SPFFT_SUCCESS);                        \
        }                                                                                                  \
        for (int rep = 0; rep < 2; ++rep) {                                                                \
          for (int i = 0; i < NS; ++i) r[i] = (REAL)(0.125 * (i % 5));                                     \
          CHECK(DENSITY_FAN(NT, ts, v, kin, c, ws, r) == SPFFT_SUCCESS);                                   \
          const double err = NAME##_err(r, NAME##_rhoref, NS);                                             \
          printf("density_fan %s %s complex %d null %d rep %d: max rel error %.3e\n", #REAL, where, c,     \
                 nul, rep, err);                                                                           \
          CHECK(err < TOL);                                                                                \
        }                                                                                                  \
        for (int s = 0; s < 2; ++s) {                                                                      \
          const SpfftScalingType scaling = s ? SPFFT_FULL_SCALING : SPFFT_NO_SCALING;                      \
          for (int t = 0; t < NT; ++t) {                                                                   \
            NAME##_mul(NAME##_pre, v, kin[t], c, nv, 0);                                                   \
            CHECK(APPLY(ts[t], NAME##_pre, vs[t], NAME##_res, scaling) == SPFFT_SUCCESS);                  \
            NAME##_mul(NAME##_ref, NAME##_res, kout[t], c, nv, t > 0);                                     \
          }                                                                                                \
          for (int rep = 0; rep < 2; ++rep) {                                                              \
            for (int i = 0; i < 2 * nv; ++i) o[i] = (REAL)-1;                                              \
            CHECK(APPLY_FAN(NT, ts, v, kin, vs, kout, c, o, scaling) == SPFFT_SUCCESS);                    \
            const double err = NAME##_err(o, NAME##_ref, 2 * nv);                                          \
            printf("apply_local_fan %s %s complex %d null %d scaling %d rep %d: max rel error %.3e\n",     \
                   #REAL, where, c, nul, s, rep, err);                                                     \
            CHECK(err < TOL);                                                                              \
          }                                                                                                \
          /* input == output */                                                                            \
          for (int i = 0; i < 2 * nv; ++i) o[i] = v[i];                                                    \
          CHECK(APPLY_FAN(NT, ts, o, kin, vs, kout, c, o, scaling) == SPFFT_SUCCESS);                      \
          CHECK(NAME##_err(o, NAME##_ref, 2 * nv) < TOL);                                                  \
        }                                                                                                  \
      }                                                                                                    \
    /* n = 1 with null kernels: the single calls */                                                        \
    CHECK(APPLY(ts[0], v, vs[0], NAME##_ref, SPFFT_FULL_SCALING) == SPFFT_SUCCESS);                        \
    CHECK(APPLY_FAN(1, ts, v, none3, vs, none3, 0, o, SPFFT_FULL_SCALING) == SPFFT_SUCCESS);               \
    CHECK(NAME##_err(o, NAME##_ref, 2 * nv) < TOL);                                                        \
    for (int i = 0; i < NS; ++i) r[i] = NAME##_rhoref[i] = (REAL)0;                                        \
    CHECK(DENSITY(ts[0], v, ws[1], NAME##_rhoref) == SPFFT_SUCCESS);                                       \
    CHECK(DENSITY_FAN(1, ts, v, none3, 0, ws + 1, r) == SPFFT_SUCCESS);                                    \
    CHECK(NAME##_err(r, NAME##_rhoref, NS) < TOL);                                                         \
    for (int t = 0; t < NT; ++t) DESTROY(ts[t]);                                                           \
    DESTROY(other);                                                                                        \
  }

DEFINE_RUN(run_double, double, SpfftGrid, SpfftTransform, spfft_grid_create, spfft_grid_destroy,
           spfft_transform_create, spfft_transform_clone, spfft_transform_destroy,
           spfft_amd_transform_apply_local, spfft_amd_transform_accumulate_density,
           spfft_amd_multi_transform_accumulate_density_fan, spfft_amd_multi_transform_apply_local_fan,
           spfft_amd_transform_values_fan_fused, 1e-12)
DEFINE_RUN(run_float, float, SpfftFloatGrid, SpfftFloatTransform, spfft_float_grid_create,
           spfft_float_grid_destroy, spfft_float_transform_create, spfft_float_transform_clone,
           spfft_float_transform_destroy, spfft_amd_float_transform_apply_local,
           spfft_amd_float_transform_accumulate_density,
           spfft_amd_float_multi_transform_accumulate_density_fan,
           spfft_amd_float_multi_transform_apply_local_fan, spfft_amd_float_transform_values_fan_fused, 2e-5)

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
