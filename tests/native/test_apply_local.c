/* spfft_amd_transform_apply_local through the C API: a full 4x3x2 index set and
 * the potential V(x) = 1 + cos(2 pi x / 4), whose product in real space is the
 * convolution out[k] = in[k] + (in[k - ex] + in[k + ex]) / 2 of the frequency
 * values (full scaling); a null potential must be an invalid-parameter error.
 * Runs on the host engine and, when a device is visible, on the GPU (fused). */
#include <math.h>
#include <stdio.h>

#include "spfft/amd.h"
#include "spfft/spfft.h"

#define NX 4
#define NY 3
#define NZ 2
#define NV (NX * NY * NZ)

static int failed = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL line %d: %s\n", __LINE__, #cond);              \
      ++failed;                                                   \
    }                                                             \
  } while (0)

static int at(int x, int y, int z) { return ((x + NX) % NX * NY + y) * NZ + z; }

static void run(SpfftProcessingUnitType pu, int expectFused) {
  int indices[3 * NV];
  double in[2 * NV], out[2 * NV], pot[NV];
  const double pi = 3.14159265358979323846;
  for (int x = 0; x < NX; ++x)
    for (int y = 0; y < NY; ++y)
      for (int z = 0; z < NZ; ++z) {
        const int i = at(x, y, z);
        indices[3 * i] = x;
        indices[3 * i + 1] = y;
        indices[3 * i + 2] = z;
        in[2 * i] = 1.0 + i;
        in[2 * i + 1] = 0.5 - 0.25 * i;
        /* space domain layout [z][y][x] */
        pot[(z * NY + y) * NX + x] = 1.0 + cos(2.0 * pi * x / NX);
      }
  SpfftGrid grid = NULL;
  SpfftTransform t = NULL;
  CHECK(spfft_grid_create(&grid, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);
  CHECK(spfft_transform_create(&t, grid, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, NV,
                               SPFFT_INDEX_TRIPLETS, indices) == SPFFT_SUCCESS);
  spfft_grid_destroy(grid);
  if (!t) return;
  int fused = -1;
  CHECK(spfft_amd_transform_apply_local_fused(t, &fused) == SPFFT_SUCCESS);
  CHECK(fused == expectFused);
  CHECK(spfft_amd_transform_apply_local(t, in, NULL, out, SPFFT_FULL_SCALING) ==
        SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_apply_local(NULL, in, pot, out, SPFFT_FULL_SCALING) ==
        SPFFT_INVALID_HANDLE_ERROR);
  for (int rep = 0; rep < 2; ++rep) {
    CHECK(spfft_amd_transform_apply_local(t, in, pot, out, SPFFT_FULL_SCALING) == SPFFT_SUCCESS);
    double err = 0;
    for (int x = 0; x < NX; ++x)
      for (int y = 0; y < NY; ++y)
        for (int z = 0; z < NZ; ++z)
          for (int c = 0; c < 2; ++c) {
            const double want = in[2 * at(x, y, z) + c] +
                                0.5 * (in[2 * at(x - 1, y, z) + c] + in[2 * at(x + 1, y, z) + c]);
            err = fmax(err, fabs(out[2 * at(x, y, z) + c] - want));
          }
    printf("apply_local %s rep %d: max abs error %.3e\n", pu == SPFFT_PU_GPU ? "gpu" : "host", rep,
           err);
    CHECK(err < 1e-12);
  }
  /* in place: output == input */
  CHECK(spfft_amd_transform_apply_local(t, in, pot, in, SPFFT_FULL_SCALING) == SPFFT_SUCCESS);
  double err = 0;
  for (int i = 0; i < 2 * NV; ++i) err = fmax(err, fabs(in[i] - out[i]));
  CHECK(err < 1e-12);
  spfft_transform_destroy(t);
}

int main(void) {
  run(SPFFT_PU_HOST, 0);
  if (spfft_amd_device_count() > 0)
    run(SPFFT_PU_GPU, 1);
  else
    printf("SKIP gpu (no device)\n");
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
