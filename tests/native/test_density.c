/* spfft_amd_transform_accumulate_density through the C API: a sparse 6x5x4
 * index set, rho += w |backward(values)|^2 against the direct O(N^2) sum, twice
 * (the second call on top of the first, with a negative weight), and once more
 * through the multi-transform entry point; a null density and a null handle
 * must be errors. Runs on the host engine and, when a device is visible, on the
 * GPU (fused). */
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
static void* const float_symbols[] = {(void*)spfft_amd_float_transform_accumulate_density,
                                      (void*)spfft_amd_float_transform_density_fused,
                                      (void*)spfft_amd_float_multi_transform_accumulate_density};

static void run(SpfftProcessingUnitType pu, int expectFused) {
  static int indices[3 * NS];
  static double in[2 * NS], rho[NS], want[NS], mod2[NS];
  const double pi = 3.14159265358979323846;
  int nv = 0;
  for (int x = 0; x < NX; ++x)
    for (int y = 0; y < NY; ++y)
      for (int z = 0; z < NZ; ++z) {
        if ((x + 2 * y) % 4 == 3) continue; /* whole sticks left out */
        indices[3 * nv] = x;
        indices[3 * nv + 1] = y;
        indices[3 * nv + 2] = z;
        in[2 * nv] = 1.0 + 0.125 * nv;
        in[2 * nv + 1] = 0.5 - 0.25 * (nv % 7);
        ++nv;
      }
  /* |direct backward sum|^2, space domain layout [z][y][x] */
  for (int z = 0; z < NZ; ++z)
    for (int y = 0; y < NY; ++y)
      for (int x = 0; x < NX; ++x) {
        double re = 0, im = 0;
        for (int k = 0; k < nv; ++k) {
          const double ph = 2.0 * pi *
                            ((double)indices[3 * k] * x / NX + (double)indices[3 * k + 1] * y / NY +
                             (double)indices[3 * k + 2] * z / NZ);
          re += in[2 * k] * cos(ph) - in[2 * k + 1] * sin(ph);
          im += in[2 * k] * sin(ph) + in[2 * k + 1] * cos(ph);
        }
        const int i = (z * NY + y) * NX + x;
        mod2[i] = re * re + im * im;
        rho[i] = want[i] = 0.25 * i - 3.0;
      }
  SpfftGrid grid = NULL;
  SpfftTransform t = NULL;
  CHECK(spfft_grid_create(&grid, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);
  CHECK(spfft_transform_create(&t, grid, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv,
                               SPFFT_INDEX_TRIPLETS, indices) == SPFFT_SUCCESS);
  spfft_grid_destroy(grid);
  if (!t) return;
  int fused = -1;
  CHECK(spfft_amd_transform_density_fused(t, &fused) == SPFFT_SUCCESS);
  CHECK(fused == expectFused);
  CHECK(spfft_amd_transform_density_fused(t, NULL) == SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_accumulate_density(t, in, 1.0, NULL) == SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_accumulate_density(NULL, in, 1.0, rho) == SPFFT_INVALID_HANDLE_ERROR);
  const double weights[3] = {0.75, -0.5, 2.0};
  double scale = 0;
  for (int i = 0; i < NS; ++i) scale = fmax(scale, mod2[i]);
  for (int rep = 0; rep < 3; ++rep) {
    if (rep < 2) {
      CHECK(spfft_amd_transform_accumulate_density(t, in, weights[rep], rho) == SPFFT_SUCCESS);
    } else {
      const double* ins[1] = {in};
      CHECK(spfft_amd_multi_transform_accumulate_density(1, &t, ins, &weights[rep], rho) ==
            SPFFT_SUCCESS);
      CHECK(spfft_amd_multi_transform_accumulate_density(1, &t, ins, &weights[rep], NULL) ==
            SPFFT_INVALID_PARAMETER_ERROR);
    }
    double err = 0;
    for (int i = 0; i < NS; ++i) {
      want[i] += weights[rep] * mod2[i];
      err = fmax(err, fabs(rho[i] - want[i]));
    }
    printf("accumulate_density %s rep %d: max rel error %.3e\n", pu == SPFFT_PU_GPU ? "gpu" : "host",
           rep, err / scale);
    CHECK(err / scale < 1e-12);
  }
  spfft_transform_destroy(t);
}

int main(void) {
  CHECK(float_symbols[0] && float_symbols[1] && float_symbols[2]);
  run(SPFFT_PU_HOST, 0);
  if (spfft_amd_device_count() > 0)
    run(SPFFT_PU_GPU, 1);
  else
    printf("SKIP gpu (no device)\n");
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
