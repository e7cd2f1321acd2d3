/* spfft_amd_transform_apply_reciprocal through the C API: a sparse 6x5x4 index
 * set, space = backward(K * scale * forward(space)) against the direct O(N^2)
 * sums, with a real and with a complex kernel, both scalings, with and without
 * the values output, each twice; a null kernel, a bad scaling, a null handle
 * and a null fused pointer must be errors and leave the transform usable. Runs
 * on the host engine and, when a device is visible, on the GPU (fused). */
#include <math.h>
#include <stdio.h>

#include "spfft/amd.h"
#include "spfft/spfft.h"

#define NX 6
#define NY 5
#define NZ 4
#define NS (NX * NY * NZ)

static int failed = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL line %d: %s\n", __LINE__, #cond);              \
      ++failed;                                                   \
    }                                                             \
  } while (0)

/* the float entry points must be exported too */
static void* const float_symbols[] = {(void*)spfft_amd_float_transform_apply_reciprocal,
                                      (void*)spfft_amd_float_transform_reciprocal_fused};

static int indices[3 * NS];
static double f[2 * NS], kern[2 * NS], kreal[NS], freq[2 * NS], want[2 * NS], values[2 * NS];

static double phase(int k, int x, int y, int z) {
  const double pi = 3.14159265358979323846;
  return 2.0 * pi *
         ((double)indices[3 * k] * x / NX + (double)indices[3 * k + 1] * y / NY +
          (double)indices[3 * k + 2] * z / NZ);
}

/* freq = scale * forward(f) on the index set; want = backward(K * freq) */
static void direct(int nv, int complexKernel, double scale) {
  for (int k = 0; k < nv; ++k) {
    double re = 0, im = 0;
    for (int z = 0; z < NZ; ++z)
      for (int y = 0; y < NY; ++y)
        for (int x = 0; x < NX; ++x) {
          const int i = (z * NY + y) * NX + x;
          const double ph = -phase(k, x, y, z);
          re += f[2 * i] * cos(ph) - f[2 * i + 1] * sin(ph);
          im += f[2 * i] * sin(ph) + f[2 * i + 1] * cos(ph);
        }
    freq[2 * k] = scale * re;
    freq[2 * k + 1] = scale * im;
  }
  for (int z = 0; z < NZ; ++z)
    for (int y = 0; y < NY; ++y)
      for (int x = 0; x < NX; ++x) {
        double re = 0, im = 0;
        for (int k = 0; k < nv; ++k) {
          const double kr = complexKernel ? kern[2 * k] : kreal[k];
          const double ki = complexKernel ? kern[2 * k + 1] : 0.0;
          const double vr = freq[2 * k] * kr - freq[2 * k + 1] * ki;
          const double vi = freq[2 * k] * ki + freq[2 * k + 1] * kr;
          const double ph = phase(k, x, y, z);
          re += vr * cos(ph) - vi * sin(ph);
          im += vr * sin(ph) + vi * cos(ph);
        }
        const int i = (z * NY + y) * NX + x;
        want[2 * i] = re;
        want[2 * i + 1] = im;
      }
}

static double max_abs(const double* a, int n) {
  double m = 0;
  for (int i = 0; i < n; ++i) m = fmax(m, fabs(a[i]));
  return m;
}

static double max_diff(const double* a, const double* b, int n) {
  double m = 0;
  for (int i = 0; i < n; ++i) m = fmax(m, fabs(a[i] - b[i]));
  return m;
}

static void run(SpfftProcessingUnitType pu, int expectFused) {
  const char* name = pu == SPFFT_PU_GPU ? "gpu" : "host";
  int nv = 0;
  for (int x = 0; x < NX; ++x)
    for (int y = 0; y < NY; ++y)
      for (int z = 0; z < NZ; ++z) {
        if ((x + 2 * y) % 4 == 3) continue; /* whole sticks left out */
        indices[3 * nv] = x;
        indices[3 * nv + 1] = y;
        indices[3 * nv + 2] = z;
        kreal[nv] = 1.0 / (1.0 + 0.5 * x + 0.25 * y + 0.125 * z);
        kern[2 * nv] = 0.5 + 0.0625 * (nv % 5);
        kern[2 * nv + 1] = 0.25 - 0.125 * (nv % 3);
        ++nv;
      }
  SpfftGrid grid = NULL;
  SpfftTransform t = NULL;
  CHECK(spfft_grid_create(&grid, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);
  CHECK(spfft_transform_create(&t, grid, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv,
                               SPFFT_INDEX_TRIPLETS, indices) == SPFFT_SUCCESS);
  spfft_grid_destroy(grid);
  if (!t) return;
  double* space = NULL;
  CHECK(spfft_transform_get_space_domain(t, SPFFT_PU_HOST, &space) == SPFFT_SUCCESS);
  if (!space) return;
  int fused = -1;
  CHECK(spfft_amd_transform_reciprocal_fused(t, &fused) == SPFFT_SUCCESS);
  CHECK(fused == expectFused);
  CHECK(spfft_amd_transform_reciprocal_fused(t, NULL) == SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_reciprocal_fused(NULL, &fused) == SPFFT_INVALID_HANDLE_ERROR);
  CHECK(spfft_amd_transform_apply_reciprocal(t, SPFFT_PU_HOST, NULL, 0, NULL, SPFFT_NO_SCALING) ==
        SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_apply_reciprocal(t, SPFFT_PU_HOST, kreal, 0, NULL,
                                             (SpfftScalingType)7) == SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_apply_reciprocal(NULL, SPFFT_PU_HOST, kreal, 0, NULL,
                                             SPFFT_NO_SCALING) == SPFFT_INVALID_HANDLE_ERROR);
  for (int c = 0; c < 2; ++c)
    for (int s = 0; s < 2; ++s) {
      const SpfftScalingType scaling = s ? SPFFT_FULL_SCALING : SPFFT_NO_SCALING;
      for (int i = 0; i < NS; ++i) {
        f[2 * i] = 1.0 + 0.125 * (i % 11) - 0.01 * i;
        f[2 * i + 1] = 0.5 - 0.25 * (i % 7);
      }
      direct(nv, c, s ? 1.0 / NS : 1.0);
      const double refSpace = max_abs(want, 2 * NS), refFreq = max_abs(freq, 2 * nv);
      for (int rep = 0; rep < 2; ++rep) {
        for (int i = 0; i < 2 * NS; ++i) space[i] = f[i];
        for (int i = 0; i < 2 * nv; ++i) values[i] = -1.0;
        double* out = rep == 0 ? values : NULL; /* second call without the values output */
        CHECK(spfft_amd_transform_apply_reciprocal(t, SPFFT_PU_HOST, c ? kern : kreal, c, out,
                                                   scaling) == SPFFT_SUCCESS);
        const double err = max_diff(space, want, 2 * NS) / refSpace;
        printf("apply_reciprocal %s complex %d scaling %d rep %d: max rel error %.3e\n", name, c, s,
               rep, err);
        CHECK(err < 1e-12);
        if (out) {
          const double verr = max_diff(values, freq, 2 * nv) / refFreq;
          printf("apply_reciprocal %s values: max rel error %.3e\n", name, verr);
          CHECK(verr < 1e-12);
        }
      }
    }
  spfft_transform_destroy(t);
}

int main(void) {
  CHECK(float_symbols[0] && float_symbols[1]);
  run(SPFFT_PU_HOST, 0);
  if (spfft_amd_device_count() > 0)
    run(SPFFT_PU_GPU, 1);
  else
    printf("SKIP gpu (no device)\n");
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
