/* spfft_amd_transform_fock_r2c_fused and spfft_amd_transform_accumulate_fock on
 * R2C transforms through the C API: both precisions export the query; a null
 * fused pointer and a null handle are errors; a host R2C transform reports 0.
 * When a device is visible a 64x13x5 R2C GPU transform reports 1 (the
 * packed-real pair x stages), and its accumulate_fock with host pointers, with a
 * real and with a hermitian complex kernel, both scalings, on two consecutive
 * calls, agrees with the direct composition on a second transform: the product
 * a * b written to the space domain, the public forward, a host loop over the
 * values, the public backward and a host loop acc += w * a * space. */
#include <math.h>
#include <stdio.h>

#include "spfft/amd.h"
#include "spfft/spfft.h"

#define NX 64
#define NY 13
#define NZ 5
#define NH (NX / 2 + 1)
#define NS (NX * NY * NZ)
#define NV (NH * NY * NZ)

static int failed = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL line %d: %s\n", __LINE__, #cond);              \
      ++failed;                                                   \
    }                                                             \
  } while (0)

/* the float entry points must be exported too */
static void* const float_symbols[] = {(void*)spfft_amd_float_transform_fock_r2c_fused,
                                      (void*)spfft_amd_float_transform_accumulate_fock};

static int indices[3 * NV];
static double a[NS], b[NS], a0[NS], b0[NS], kern[2 * NV], kreal[NV];
static double freq[2 * NV], upd[NS], acc[NS], acc0[NS], want[NS], values[2 * NV];

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

static int signed_index(int i, int n) { return i <= n / 2 ? i : i - n; }

/* the whole hermitian half: x = 0..NX/2, every y and z; kernels with K(-G) =
 * conj(K(G)), so that the update of real fields is real */
static int fill_indices(void) {
  const double pi = 3.14159265358979323846;
  int nv = 0;
  for (int x = 0; x < NH; ++x)
    for (int y = 0; y < NY; ++y)
      for (int z = 0; z < NZ; ++z) {
        const int gy = signed_index(y, NY), gz = signed_index(z, NZ);
        indices[3 * nv] = x;
        indices[3 * nv + 1] = y;
        indices[3 * nv + 2] = z;
        kreal[nv] = 1.0 / (1.0 + 0.5 * x * x + 0.25 * gy * gy + 0.125 * gz * gz);
        const double ph = -2.0 * pi * (3.0 * x / NX + 2.0 * gy / NY + 1.0 * gz / NZ);
        kern[2 * nv] = kreal[nv] * cos(ph);
        kern[2 * nv + 1] = kreal[nv] * sin(ph);
        ++nv;
      }
  return nv;
}

static SpfftTransform create(SpfftProcessingUnitType pu, int nv) {
  SpfftGrid grid = NULL;
  SpfftTransform t = NULL;
  CHECK(spfft_grid_create(&grid, NX, NY, NZ, NH * NY, pu, -1) == SPFFT_SUCCESS);
  CHECK(spfft_transform_create(&t, grid, pu, SPFFT_TRANS_R2C, NX, NY, NZ, NZ, nv, SPFFT_INDEX_TRIPLETS,
                               indices) == SPFFT_SUCCESS);
  spfft_grid_destroy(grid);
  return t;
}

/* freq = scale * forward(a b); upd = w a backward(K freq): public transforms
 * and host loops */
static void direct(SpfftTransform ref, int nv, int complexKernel, SpfftScalingType scaling, double w) {
  double* space = NULL;
  CHECK(spfft_transform_get_space_domain(ref, SPFFT_PU_HOST, &space) == SPFFT_SUCCESS);
  if (!space) return;
  for (int i = 0; i < NS; ++i) space[i] = a[i] * b[i];
  CHECK(spfft_transform_forward(ref, SPFFT_PU_HOST, freq, scaling) == SPFFT_SUCCESS);
  for (int k = 0; k < nv; ++k) {
    const double kr = complexKernel ? kern[2 * k] : kreal[k];
    const double ki = complexKernel ? kern[2 * k + 1] : 0.0;
    values[2 * k] = freq[2 * k] * kr - freq[2 * k + 1] * ki;
    values[2 * k + 1] = freq[2 * k] * ki + freq[2 * k + 1] * kr;
  }
  CHECK(spfft_transform_backward(ref, values, SPFFT_PU_HOST) == SPFFT_SUCCESS);
  for (int i = 0; i < NS; ++i) upd[i] = w * a[i] * space[i];
}

static void run_gpu(int nv) {
  const double w = -0.75;
  for (int i = 0; i < NS; ++i) {
    a[i] = a0[i] = 1.0 + 0.125 * (i % 11) - 0.0001 * i;
    b[i] = b0[i] = -0.75 + 0.25 * (i % 5) + 0.03125 * (i % 13);
  }
  SpfftTransform t = create(SPFFT_PU_GPU, nv);
  SpfftTransform ref = create(SPFFT_PU_GPU, nv);
  if (!t || !ref) return;
  int fused = -1;
  CHECK(spfft_amd_transform_fock_r2c_fused(t, &fused) == SPFFT_SUCCESS);
  CHECK(fused == 1);
  fused = -1;
  CHECK(spfft_amd_transform_fock_fused(t, &fused) == SPFFT_SUCCESS);
  CHECK(fused == 0);
  for (int c = 0; c < 2; ++c)
    for (int s = 0; s < 2; ++s) {
      const SpfftScalingType scaling = s ? SPFFT_FULL_SCALING : SPFFT_NO_SCALING;
      direct(ref, nv, c, scaling, w);
      const double refUpd = max_abs(upd, NS), refFreq = max_abs(freq, 2 * nv);
      CHECK(refUpd > 0.0);
      for (int i = 0; i < NS; ++i) {
        acc0[i] = refUpd * (0.5 - 0.0625 * (i % 17)); /* of the update's size */
        acc[i] = acc0[i];
      }
      for (int rep = 0; rep < 2; ++rep) {
        for (int i = 0; i < 2 * nv; ++i) values[i] = -1.0;
        double* out = rep == 0 ? values : NULL; /* second call without the values output */
        CHECK(spfft_amd_transform_accumulate_fock(t, a, b, c ? kern : kreal, c, w, acc, out, scaling) ==
              SPFFT_SUCCESS);
        double eUpd = 0;
        for (int i = 0; i < NS; ++i) {
          want[i] = acc0[i] + (rep + 1) * upd[i];
          eUpd = fmax(eUpd, fabs((acc[i] - acc0[i]) - (rep + 1) * upd[i]));
        }
        const double eAcc = max_diff(acc, want, NS) / max_abs(want, NS);
        eUpd /= (rep + 1) * refUpd;
        printf("accumulate_fock r2c gpu complex %d scaling %d rep %d: max rel error acc %.3e update %.3e\n", c, s,
               rep, eAcc, eUpd);
        CHECK(eAcc < 1e-12);
        CHECK(eUpd < 1e-12);
        if (out) {
          const double verr = max_diff(values, freq, 2 * nv) / refFreq;
          printf("accumulate_fock r2c gpu values: max rel error %.3e\n", verr);
          CHECK(verr < 1e-12);
        }
        CHECK(max_diff(a, a0, NS) == 0.0 && max_diff(b, b0, NS) == 0.0);
      }
    }
  spfft_transform_destroy(ref);
  spfft_transform_destroy(t);
}

int main(void) {
  CHECK(float_symbols[0] && float_symbols[1]);
  const int nv = fill_indices();
  int fused = -1;
  CHECK(spfft_amd_transform_fock_r2c_fused(NULL, &fused) == SPFFT_INVALID_HANDLE_ERROR);
  CHECK(spfft_amd_float_transform_fock_r2c_fused(NULL, &fused) == SPFFT_INVALID_HANDLE_ERROR);
  SpfftTransform host = create(SPFFT_PU_HOST, nv);
  if (host) {
    CHECK(spfft_amd_transform_fock_r2c_fused(host, NULL) == SPFFT_INVALID_PARAMETER_ERROR);
    fused = -1;
    CHECK(spfft_amd_transform_fock_r2c_fused(host, &fused) == SPFFT_SUCCESS);
    CHECK(fused == 0);
    printf("fock_r2c_fused host: %d\n", fused);
    spfft_transform_destroy(host);
  }
  if (spfft_amd_device_count() > 0)
    run_gpu(nv);
  else
    printf("SKIP gpu (no device)\n");
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
