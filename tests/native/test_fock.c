/* spfft_amd_transform_accumulate_fock through the C API: a sparse 6x5x4 index
 * set, acc += w * a * backward(K * scale * forward(conj(a) * b)) against the
 * direct O(N^2) sums, with a real and with a complex kernel, both scalings,
 * with and without the values output, each on two consecutive calls; a null
 * acc, a null kernel, a bad scaling, a null handle and a null fused pointer
 * must be errors and leave the transform usable. Runs on the host engine and,
 * when a device is visible, on the GPU (fused x stages, host pointers). */
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
static void* const float_symbols[] = {(void*)spfft_amd_float_transform_accumulate_fock,
                                      (void*)spfft_amd_float_transform_fock_fused};

static int indices[3 * NS];
static double a[2 * NS], b[2 * NS], a0[2 * NS], b0[2 * NS], pair[2 * NS], kern[2 * NS], kreal[NS];
static double freq[2 * NS], upd[2 * NS], acc[2 * NS], acc0[2 * NS], want[2 * NS], values[2 * NS];

static double phase(int k, int x, int y, int z) {
  const double pi = 3.14159265358979323846;
  return 2.0 * pi *
         ((double)indices[3 * k] * x / NX + (double)indices[3 * k + 1] * y / NY +
          (double)indices[3 * k + 2] * z / NZ);
}

/* freq = scale * forward(conj(a) b) on the index set; upd = w a backward(K freq) */
static void direct(int nv, int complexKernel, double scale, double w) {
  for (int i = 0; i < NS; ++i) {
    pair[2 * i] = a[2 * i] * b[2 * i] + a[2 * i + 1] * b[2 * i + 1];
    pair[2 * i + 1] = a[2 * i] * b[2 * i + 1] - a[2 * i + 1] * b[2 * i];
  }
  for (int k = 0; k < nv; ++k) {
    double re = 0, im = 0;
    for (int z = 0; z < NZ; ++z)
      for (int y = 0; y < NY; ++y)
        for (int x = 0; x < NX; ++x) {
          const int i = (z * NY + y) * NX + x;
          const double ph = -phase(k, x, y, z);
          re += pair[2 * i] * cos(ph) - pair[2 * i + 1] * sin(ph);
          im += pair[2 * i] * sin(ph) + pair[2 * i + 1] * cos(ph);
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
        upd[2 * i] = w * (a[2 * i] * re - a[2 * i + 1] * im);
        upd[2 * i + 1] = w * (a[2 * i] * im + a[2 * i + 1] * re);
      }
}

static double max_abs(const double* p, int n) {
  double m = 0;
  for (int i = 0; i < n; ++i) m = fmax(m, fabs(p[i]));
  return m;
}

static double max_diff(const double* p, const double* q, int n) {
  double m = 0;
  for (int i = 0; i < n; ++i) m = fmax(m, fabs(p[i] - q[i]));
  return m;
}

static void run(SpfftProcessingUnitType pu, int expectFused) {
  const char* name = pu == SPFFT_PU_GPU ? "gpu" : "host";
  const double w = -0.75;
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
  for (int i = 0; i < NS; ++i) {
    a[2 * i] = a0[2 * i] = 1.0 + 0.125 * (i % 11) - 0.01 * i;
    a[2 * i + 1] = a0[2 * i + 1] = 0.5 - 0.25 * (i % 7);
    b[2 * i] = b0[2 * i] = -0.75 + 0.25 * (i % 5);
    b[2 * i + 1] = b0[2 * i + 1] = 0.125 * (i % 13) - 0.5;
  }
  SpfftGrid grid = NULL;
  SpfftTransform t = NULL;
  CHECK(spfft_grid_create(&grid, NX, NY, NZ, NX * NY, pu, -1) == SPFFT_SUCCESS);
  CHECK(spfft_transform_create(&t, grid, pu, SPFFT_TRANS_C2C, NX, NY, NZ, NZ, nv,
                               SPFFT_INDEX_TRIPLETS, indices) == SPFFT_SUCCESS);
  spfft_grid_destroy(grid);
  if (!t) return;
  int fused = -1;
  CHECK(spfft_amd_transform_fock_fused(t, &fused) == SPFFT_SUCCESS);
  CHECK(fused == expectFused);
  CHECK(spfft_amd_transform_fock_fused(t, NULL) == SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_fock_fused(NULL, &fused) == SPFFT_INVALID_HANDLE_ERROR);
  CHECK(spfft_amd_transform_accumulate_fock(t, a, b, kreal, 0, w, NULL, NULL, SPFFT_NO_SCALING) ==
        SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_accumulate_fock(t, a, b, NULL, 0, w, acc, NULL, SPFFT_NO_SCALING) ==
        SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_accumulate_fock(t, NULL, b, kreal, 0, w, acc, NULL, SPFFT_NO_SCALING) ==
        SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_accumulate_fock(t, a, NULL, kreal, 0, w, acc, NULL, SPFFT_NO_SCALING) ==
        SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_accumulate_fock(t, a, b, kreal, 0, w, acc, NULL, (SpfftScalingType)7) ==
        SPFFT_INVALID_PARAMETER_ERROR);
  CHECK(spfft_amd_transform_accumulate_fock(NULL, a, b, kreal, 0, w, acc, NULL, SPFFT_NO_SCALING) ==
        SPFFT_INVALID_HANDLE_ERROR);
  for (int c = 0; c < 2; ++c)
    for (int s = 0; s < 2; ++s) {
      const SpfftScalingType scaling = s ? SPFFT_FULL_SCALING : SPFFT_NO_SCALING;
      direct(nv, c, s ? 1.0 / NS : 1.0, w);
      const double refUpd = max_abs(upd, 2 * NS), refFreq = max_abs(freq, 2 * nv);
      for (int i = 0; i < 2 * NS; ++i) {
        acc0[i] = refUpd * (0.5 - 0.0625 * (i % 17)); /* of the update's size */
        acc[i] = acc0[i];
      }
      for (int rep = 0; rep < 2; ++rep) {
        for (int i = 0; i < 2 * nv; ++i) values[i] = -1.0;
        double* out = rep == 0 ? values : NULL; /* second call without the values output */
        CHECK(spfft_amd_transform_accumulate_fock(t, a, b, c ? kern : kreal, c, w, acc, out,
                                                  scaling) == SPFFT_SUCCESS);
        /* the whole acc, and the update alone, after rep + 1 calls */
        double eAcc = 0, eUpd = 0;
        for (int i = 0; i < 2 * NS; ++i) {
          want[i] = acc0[i] + (rep + 1) * upd[i];
          eUpd = fmax(eUpd, fabs((acc[i] - acc0[i]) - (rep + 1) * upd[i]));
        }
        eAcc = max_diff(acc, want, 2 * NS) / max_abs(want, 2 * NS);
        eUpd /= (rep + 1) * refUpd;
        printf("accumulate_fock %s complex %d scaling %d rep %d: max rel error acc %.3e update %.3e\n",
               name, c, s, rep, eAcc, eUpd);
        CHECK(eAcc < 1e-12);
        CHECK(eUpd < 1e-12);
        if (out) {
          const double verr = max_diff(values, freq, 2 * nv) / refFreq;
          printf("accumulate_fock %s values: max rel error %.3e\n", name, verr);
          CHECK(verr < 1e-12);
        }
        CHECK(max_diff(a, a0, 2 * NS) == 0.0 && max_diff(b, b0, 2 * NS) == 0.0);
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
