/* spfft_amd_multi_transform_apply_local_spinor / accumulate_spin_density and
 * their float twins through the C API: two spinors (a transform and three
 * clones, in the order up_0, dn_0, up_1, dn_1) on a sparse 6x5x4 index set, on
 * two consecutive calls whose results must agree bit for bit, against direct
 * sums in double precision: psi = sum_G c e^{+2 pi i G r / N}, the 2x2 mix with
 * {v_uu, v_dd, v_ud_re, v_ud_im}, out = scale sum_r f e^{-2 pi i G r / N}, and
 * the density matrix {|u|^2, |d|^2, u conj(d)}; both scalings, out == in,
 * repeated potential pointers. An R2C member, a repeated grid, unequal
 * transforms, null arrays, a null input, output, potential or density entry,
 * equal density pointers, a bad scaling and a null handle must be errors and
 * leave the transforms usable; nSpinors = 0 is a no-op. Runs on the host engine
 * and, when a device is visible, on the GPU with host pointers (the composed
 * path) and with device pointers (the fused x kernels, which the query tells). */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "spfft/amd.h"
#include "spfft/spfft.h"

#define NX 6
#define NY 5
#define NZ 4
#define NS (NX * NY * NZ)
#define NSP 2
#define NT (2 * NSP)

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

/* the references, in double: space[r] = sum_k vals[k] e^{+i phase}, and back */
static double ref_space[NT][2 * NS], ref_out[NT][2 * NS], ref_dens[4][NS], ref_vals[NT][2 * NS],
    ref_pot[4][NS];

static double phase(int k, int r) {
  const int x = r % NX, y = (r / NX) % NY, z = r / (NX * NY);
  return 2.0 * 3.14159265358979323846 *
         ((double)(indices[3 * k] * x) / NX + (double)(indices[3 * k + 1] * y) / NY +
          (double)(indices[3 * k + 2] * z) / NZ);
}

static void ref_backward(int nv) {
  for (int t = 0; t < NT; ++t)
    for (int r = 0; r < NS; ++r) {
      double re = 0, im = 0;
      for (int k = 0; k < nv; ++k) {
        const double c = cos(phase(k, r)), s = sin(phase(k, r));
        re += ref_vals[t][2 * k] * c - ref_vals[t][2 * k + 1] * s;
        im += ref_vals[t][2 * k] * s + ref_vals[t][2 * k + 1] * c;
      }
      ref_space[t][2 * r] = re;
      ref_space[t][2 * r + 1] = im;
    }
}

/* sameOffDiag: the call passes v_ud_re for v_ud_im too */
static void ref_apply(int nv, int full, int sameOffDiag) {
  static double mixed[NT][2 * NS];
  for (int s = 0; s < NSP; ++s)
    for (int r = 0; r < NS; ++r) {
      const double *u = &ref_space[2 * s][2 * r], *d = &ref_space[2 * s + 1][2 * r];
      const double vuu = ref_pot[0][r], vdd = ref_pot[1][r], vre = ref_pot[2][r];
      const double vim = sameOffDiag ? vre : ref_pot[3][r];
      mixed[2 * s][2 * r] = vuu * u[0] + vre * d[0] - vim * d[1];
      mixed[2 * s][2 * r + 1] = vuu * u[1] + vre * d[1] + vim * d[0];
      mixed[2 * s + 1][2 * r] = vdd * d[0] + vre * u[0] + vim * u[1];
      mixed[2 * s + 1][2 * r + 1] = vdd * d[1] + vre * u[1] - vim * u[0];
    }
  for (int t = 0; t < NT; ++t)
    for (int k = 0; k < nv; ++k) {
      double re = 0, im = 0;
      for (int r = 0; r < NS; ++r) {
        const double c = cos(phase(k, r)), s = sin(phase(k, r));
        re += mixed[t][2 * r] * c + mixed[t][2 * r + 1] * s;
        im += mixed[t][2 * r + 1] * c - mixed[t][2 * r] * s;
      }
      ref_out[t][2 * k] = full ? re / NS : re;
      ref_out[t][2 * k + 1] = full ? im / NS : im;
    }
}

static void ref_density(const double* w) {
  for (int r = 0; r < NS; ++r) {
    for (int k = 0; k < 4; ++k) ref_dens[k][r] = 0.125 * ((r + k) % 5);
    for (int s = 0; s < NSP; ++s) {
      const double *u = &ref_space[2 * s][2 * r], *d = &ref_space[2 * s + 1][2 * r];
      ref_dens[0][r] += w[s] * (u[0] * u[0] + u[1] * u[1]);
      ref_dens[1][r] += w[s] * (d[0] * d[0] + d[1] * d[1]);
      ref_dens[2][r] += w[s] * (u[0] * d[0] + u[1] * d[1]);
      ref_dens[3][r] += w[s] * (u[1] * d[0] - u[0] * d[1]);
    }
  }
}

static void* to_device(const void* host, size_t bytes) {
  void* p = NULL;
  CHECK(hipMalloc(&p, bytes) == hipSuccess);
  if (p) CHECK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) == hipSuccess);
  return p;
}

/* one body per precision: REAL, the handle types and the entry points.
 * device: the arrays of the calls live in device memory */
#define DEFINE_RUN(NAME, REAL, GRID, TRANSFORM, GRID_CREATE, GRID_DESTROY, CREATE, CLONE, DESTROY, APPLY,  \
                   DENSITY, QUERY, TOL)                                                                    \
  static REAL NAME##_vals[NT][2 * NS], NAME##_pot[4][NS], NAME##_out[NT][2 * NS], NAME##_dens[4][NS],      \
      NAME##_first[NT][2 * NS], NAME##_dfirst[4][NS];                                                      \
  static double NAME##_err(const REAL* got, const double* want, int count) {                               \
    double num = 0, den = 0;                                                                               \
    for (int i = 0; i < count; ++i) {                                                                      \
      num = fmax(num, fabs((double)got[i] - want[i]));                                                     \
      den = fmax(den, fabs(want[i]));                                                                      \
    }                                                                                                      \
    return den > 0 ? num / den : 1.0;                                                                      \
  }                                                                                                        \
  static void NAME(SpfftProcessingUnitType pu, int device) {                                               \
    const char* where = pu == SPFFT_PU_GPU ? (device ? "gpu-device" : "gpu-host") : "host";                \
    const int nv = make_indices();                                                                         \
    for (int t = 0; t < NT; ++t)                                                                           \
      for (int k = 0; k < nv; ++k) {                                                                       \
        NAME##_vals[t][2 * k] = (REAL)(1.0 + 0.125 * ((k + 3 * t) % 11) - 0.01 * k);                       \
        NAME##_vals[t][2 * k + 1] = (REAL)(0.5 - 0.25 * ((k + t) % 7));                                    \
        ref_vals[t][2 * k] = NAME##_vals[t][2 * k];                                                        \
        ref_vals[t][2 * k + 1] = NAME##_vals[t][2 * k + 1];                                                \
      }                                                                                                    \
    for (int c = 0; c < 4; ++c)                                                                            \
      for (int i = 0; i < NS; ++i) {                                                                       \
        NAME##_pot[c][i] = (REAL)(-1.0 + 0.125 * ((i + 5 * c) % 17));                                      \
        ref_pot[c][i] = NAME##_pot[c][i];                                                                  \
      }                                                                                                    \
    ref_backward(nv);                                                                                      \
    GRID grid = NULL, grid2 = NULL, grid3 = NULL;                                                          \
    TRANSFORM ts[NT] = {NULL, NULL, NULL, NULL};                                                           \
    TRANSFORM other = NULL, treal = NULL;                                                                  \
    CHECK(GRID_CREATE(&grid, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);                               \
    CHECK(CREATE(&ts[0], grid, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv, SPFFT_INDEX_TRIPLETS, indices) ==  \
          SPFFT_SUCCESS);                                                                                  \
    GRID_DESTROY(grid);                                                                                    \
    /* the same dimensions, fewer values; and an R2C transform (x = 0 sticks only) */                      \
    CHECK(GRID_CREATE(&grid2, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);                              \
    CHECK(CREATE(&other, grid2, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv - NZ, SPFFT_INDEX_TRIPLETS,        \
                 indices) == SPFFT_SUCCESS);                                                               \
    GRID_DESTROY(grid2);                                                                                   \
    CHECK(GRID_CREATE(&grid3, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);                              \
    CHECK(CREATE(&treal, grid3, pu, SPFFT_TRANS_R2C, NX, NY, NZ, NZ, 1, SPFFT_INDEX_TRIPLETS, indices) ==  \
          SPFFT_SUCCESS);                                                                                  \
    GRID_DESTROY(grid3);                                                                                   \
    if (!ts[0] || !other || !treal) return;                                                                \
    for (int t = 1; t < NT; ++t) CHECK(CLONE(ts[0], &ts[t]) == SPFFT_SUCCESS);                             \
    if (!ts[1] || !ts[2] || !ts[3]) return;                                                                \
    int fused = -1;                                                                                        \
    CHECK(QUERY(ts[0], &fused) == SPFFT_SUCCESS && (fused == 0 || fused == 1));                            \
    CHECK(pu == SPFFT_PU_GPU ? fused == 1 : fused == 0);                                                   \
    CHECK(QUERY(ts[0], NULL) == SPFFT_INVALID_PARAMETER_ERROR);                                            \
    CHECK(QUERY(NULL, &fused) == SPFFT_INVALID_HANDLE_ERROR);                                              \
    /* the arrays of the calls: host arrays, or device copies of them */                                   \
    REAL *in[NT], *out[NT], *pot[4], *dens[4];                                                             \
    const size_t vb = sizeof(REAL) * 2 * NS, sb = sizeof(REAL) * NS;                                       \
    for (int t = 0; t < NT; ++t) {                                                                         \
      in[t] = device ? (REAL*)to_device(NAME##_vals[t], vb) : NAME##_vals[t];                              \
      out[t] = device ? (REAL*)to_device(NAME##_out[t], vb) : NAME##_out[t];                               \
    }                                                                                                      \
    for (int c = 0; c < 4; ++c) {                                                                          \
      pot[c] = device ? (REAL*)to_device(NAME##_pot[c], sb) : NAME##_pot[c];                               \
      dens[c] = device ? (REAL*)to_device(NAME##_dens[c], sb) : NAME##_dens[c];                            \
    }                                                                                                      \
    const REAL* cin[NT] = {in[0], in[1], in[2], in[3]};                                                    \
    const REAL* cpot[4] = {pot[0], pot[1], pot[2], pot[3]};                                                \
    const REAL* prep[4] = {pot[0], pot[1], pot[2], pot[2]};                                                \
    const REAL* inhole[NT] = {in[0], NULL, in[2], in[3]};                                                  \
    REAL* outhole[NT] = {out[0], out[1], NULL, out[3]};                                                    \
    const REAL* pothole[4] = {pot[0], pot[1], NULL, pot[3]};                                               \
    REAL* denshole[4] = {dens[0], NULL, dens[2], dens[3]};                                                 \
    REAL* denstwice[4] = {dens[0], dens[1], dens[2], dens[1]};                                             \
    const REAL ws[NSP] = {(REAL)1.0, (REAL)0.5};                                                           \
    const double wd[NSP] = {1.0, 0.5};                                                                     \
    TRANSFORM twice[NT] = {ts[0], ts[1], ts[0], ts[3]};                                                    \
    TRANSFORM gap[NT] = {ts[0], NULL, ts[2], ts[3]};                                                       \
    TRANSFORM odd[NT] = {ts[0], other, ts[2], ts[3]};                                                      \
    TRANSFORM real[NT] = {ts[0], ts[1], ts[2], treal};                                                     \
    const SpfftScalingType none = SPFFT_NO_SCALING, bad = (SpfftScalingType)7;                             \
    const SpfftError inv = SPFFT_INVALID_PARAMETER_ERROR;                                                  \
    CHECK(APPLY(NSP, twice, cin, cpot, out, none) == inv);                                                 \
    CHECK(APPLY(NSP, gap, cin, cpot, out, none) == SPFFT_INVALID_HANDLE_ERROR);                            \
    CHECK(APPLY(NSP, odd, cin, cpot, out, none) == inv);                                                   \
    CHECK(APPLY(NSP, real, cin, cpot, out, none) == inv);                                                  \
    CHECK(APPLY(NSP, NULL, cin, cpot, out, none) == inv);                                                  \
    CHECK(APPLY(NSP, ts, NULL, cpot, out, none) == inv);                                                   \
    CHECK(APPLY(NSP, ts, cin, NULL, out, none) == inv);                                                    \
    CHECK(APPLY(NSP, ts, cin, cpot, NULL, none) == inv);                                                   \
    CHECK(APPLY(NSP, ts, inhole, cpot, out, none) == inv);                                                 \
    CHECK(APPLY(NSP, ts, cin, cpot, outhole, none) == inv);                                                \
    CHECK(APPLY(NSP, ts, cin, pothole, out, none) == inv);                                                 \
    CHECK(APPLY(NSP, ts, cin, cpot, out, bad) == inv);                                                     \
    CHECK(APPLY(-1, ts, cin, cpot, out, none) == inv);                                                     \
    CHECK(APPLY(0, NULL, NULL, NULL, NULL, none) == SPFFT_SUCCESS);                                        \
    CHECK(DENSITY(NSP, twice, cin, ws, dens) == inv);                                                      \
    CHECK(DENSITY(NSP, gap, cin, ws, dens) == SPFFT_INVALID_HANDLE_ERROR);                                 \
    CHECK(DENSITY(NSP, odd, cin, ws, dens) == inv);                                                        \
    CHECK(DENSITY(NSP, real, cin, ws, dens) == inv);                                                       \
    CHECK(DENSITY(NSP, NULL, cin, ws, dens) == inv);                                                       \
    CHECK(DENSITY(NSP, ts, NULL, ws, dens) == inv);                                                        \
    CHECK(DENSITY(NSP, ts, cin, NULL, dens) == inv);                                                       \
    CHECK(DENSITY(NSP, ts, cin, ws, NULL) == inv);                                                         \
    CHECK(DENSITY(NSP, ts, inhole, ws, dens) == inv);                                                      \
    CHECK(DENSITY(NSP, ts, cin, ws, denshole) == inv);                                                     \
    CHECK(DENSITY(NSP, ts, cin, ws, denstwice) == inv);                                                    \
    CHECK(DENSITY(0, NULL, NULL, NULL, NULL) == SPFFT_SUCCESS);                                            \
    /* the operator: both scalings, then repeated potential pointers, two calls each */                    \
    for (int s = 0; s < 3; ++s) {                                                                          \
      const SpfftScalingType scaling = s ? SPFFT_FULL_SCALING : SPFFT_NO_SCALING;                          \
      ref_apply(nv, s != 0, s == 2);                                                                       \
      for (int rep = 0; rep < 2; ++rep) {                                                                  \
        CHECK(APPLY(NSP, ts, cin, s == 2 ? prep : cpot, out, scaling) == SPFFT_SUCCESS);                   \
        double err = 0;                                                                                    \
        for (int t = 0; t < NT; ++t) {                                                                     \
          if (device) CHECK(hipMemcpy(NAME##_out[t], out[t], vb, hipMemcpyDeviceToHost) == hipSuccess);    \
          err = fmax(err, NAME##_err(NAME##_out[t], ref_out[t], 2 * nv));                                  \
          if (rep == 0) memcpy(NAME##_first[t], NAME##_out[t], sizeof(REAL) * 2 * nv);                     \
          else CHECK(memcmp(NAME##_first[t], NAME##_out[t], sizeof(REAL) * 2 * nv) == 0);                  \
        }                                                                                                  \
        printf("apply_local_spinor %s %s case %d rep %d: max rel error %.3e\n", #REAL, where, s, rep,      \
               err);                                                                                       \
        CHECK(err < TOL);                                                                                  \
      }                                                                                                    \
    }                                                                                                      \
    /* out == in (full scaling, the four potentials) */                                                    \
    ref_apply(nv, 1, 0);                                                                                   \
    for (int t = 0; t < NT; ++t) {                                                                         \
      if (device) CHECK(hipMemcpy(out[t], in[t], vb, hipMemcpyDeviceToDevice) == hipSuccess);              \
      else memcpy(out[t], in[t], vb);                                                                      \
    }                                                                                                      \
    {                                                                                                      \
      const REAL* same[NT] = {out[0], out[1], out[2], out[3]};                                             \
      CHECK(APPLY(NSP, ts, same, cpot, out, SPFFT_FULL_SCALING) == SPFFT_SUCCESS);                         \
      for (int t = 0; t < NT; ++t) {                                                                       \
        if (device) CHECK(hipMemcpy(NAME##_out[t], out[t], vb, hipMemcpyDeviceToHost) == hipSuccess);      \
        CHECK(NAME##_err(NAME##_out[t], ref_out[t], 2 * nv) < TOL);                                        \
      }                                                                                                    \
    }                                                                                                      \
    /* the density matrix, two calls from the same start */                                                \
    ref_density(wd);                                                                                       \
    for (int rep = 0; rep < 2; ++rep) {                                                                    \
      for (int c = 0; c < 4; ++c) {                                                                        \
        for (int i = 0; i < NS; ++i) NAME##_dens[c][i] = (REAL)(0.125 * ((i + c) % 5));                    \
        if (device) CHECK(hipMemcpy(dens[c], NAME##_dens[c], sb, hipMemcpyHostToDevice) == hipSuccess);    \
      }                                                                                                    \
      CHECK(DENSITY(NSP, ts, cin, ws, dens) == SPFFT_SUCCESS);                                             \
      double err = 0;                                                                                      \
      for (int c = 0; c < 4; ++c) {                                                                        \
        if (device) CHECK(hipMemcpy(NAME##_dens[c], dens[c], sb, hipMemcpyDeviceToHost) == hipSuccess);    \
        err = fmax(err, NAME##_err(NAME##_dens[c], ref_dens[c], NS));                                      \
        if (rep == 0) memcpy(NAME##_dfirst[c], NAME##_dens[c], sb);                                        \
        else CHECK(memcmp(NAME##_dfirst[c], NAME##_dens[c], sb) == 0);                                     \
      }                                                                                                    \
      printf("accumulate_spin_density %s %s rep %d: max rel error %.3e\n", #REAL, where, rep, err);        \
      CHECK(err < TOL);                                                                                    \
    }                                                                                                      \
    if (device) {                                                                                          \
      for (int t = 0; t < NT; ++t) {                                                                       \
        CHECK(hipFree(in[t]) == hipSuccess);                                                               \
        CHECK(hipFree(out[t]) == hipSuccess);                                                              \
      }                                                                                                    \
      for (int c = 0; c < 4; ++c) {                                                                        \
        CHECK(hipFree(pot[c]) == hipSuccess);                                                              \
        CHECK(hipFree(dens[c]) == hipSuccess);                                                             \
      }                                                                                                    \
    }                                                                                                      \
    for (int t = 0; t < NT; ++t) DESTROY(ts[t]);                                                           \
    DESTROY(other);                                                                                        \
    DESTROY(treal);                                                                                        \
  }

DEFINE_RUN(run_double, double, SpfftGrid, SpfftTransform, spfft_grid_create, spfft_grid_destroy,
           spfft_transform_create, spfft_transform_clone, spfft_transform_destroy,
           spfft_amd_multi_transform_apply_local_spinor, spfft_amd_multi_transform_accumulate_spin_density,
           spfft_amd_transform_spinor_fused, 1e-12)
DEFINE_RUN(run_float, float, SpfftFloatGrid, SpfftFloatTransform, spfft_float_grid_create,
           spfft_float_grid_destroy, spfft_float_transform_create, spfft_float_transform_clone,
           spfft_float_transform_destroy, spfft_amd_float_multi_transform_apply_local_spinor,
           spfft_amd_float_multi_transform_accumulate_spin_density, spfft_amd_float_transform_spinor_fused,
           2e-5)

int main(void) {
  run_double(SPFFT_PU_HOST, 0);
  run_float(SPFFT_PU_HOST, 0);
  if (spfft_amd_device_count() > 0) {
    run_double(SPFFT_PU_GPU, 0);
    run_float(SPFFT_PU_GPU, 0);
    run_double(SPFFT_PU_GPU, 1);
    run_float(SPFFT_PU_GPU, 1);
  } else {
    printf("SKIP gpu (no device)\n");
  }
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
