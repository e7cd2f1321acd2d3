// Kernel-argument structures and host launch entry points of the fused stage
// kernels. One kernel per stage and direction:
//   z stage: sparse values <-> z-sticks, z-FFT, (0,0)-stick hermitian fill,
//            pack into the per-rank exchange layout (replaces K4-K6, K8, K9,
//            K11, K13, K15 and the vendor z-FFT F1 of the reference).
//   y stage: exchange layout <-> [z][column][y] slab, y-FFT over x-columns that
//            hold sticks only, x=0 plane hermitian fill (replaces K2, K3, K7,
//            K10, K12, K14, K16 and half of F2/F3).
//   x stage: [z][column][y] <-> space domain [z][y][x], x-FFT C2C, C2R or R2C
//            (replaces the other half of F2/F3).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>

#include "fft/codelets.hpp"
#include "plan/index_plan.hpp"

namespace spfft {
namespace dev {

// Batched launches (multi_transform of transforms with identical plans on one
// GPU): blockIdx.z selects the transform; its input and output buffers come
// from these tables, every index table is shared. count <= 1: unbatched, the
// kernel's pointer arguments are used as given.
constexpr int kMaxBatch = 8;
struct BatchPtrs {
  int count;
  const void* in[kMaxBatch];
  void* out[kMaxBatch];
};

struct ZArgs {
  int numSticks;   // end of the stick range processed (exclusive)
  int stickBegin;  // first stick of the range (exchange pipelining chunks)
  int n;          // dimZ
  int zeroStick;  // line to hermitian-fill (R2C backward), -1 for none
  const StickRun* runs;
  const int* runOffsets;
  const StickDesc* desc;     // non-null when every stick is simple (fast path)
  int single;                // 1: exchange side is the plain [S][stickStride] array
                             // (2: distributed, segment table read from global memory)
  long long stickStride;     // element stride between sticks when single
  // otherwise, per plane z two entries: (base, stride) of its exchange segment,
  // element (stick s, plane z) at base + s * stride (base includes z)
  const long long* zTab;
  int plainSticks;  // backward: stick stores with the default cache policy (see GpuExecutor)
  // forward: streaming (nt) value stores, for value arrays larger than the
  // Infinity Cache can keep (GpuExecutor)
  int ntValueStores;
  BatchPtrs batch;
};


// A column's stick entries as at most kColRuns runs with consecutive y and
// consecutive bases: y in run r (y - y[r] < len[r]) has its entry at b0[r] +
// y * YArgs::colStride (b0 = the run's first base - y[r] * colStride). A sphere
// column is two runs (storage y = 0..h and n-h..n-1); entries from several
// ranks add runs. Workgroup-uniform, so it lives in scalar registers.
constexpr int kColRuns = 4;
struct ColDesc {
  long long b0[kColRuns];
  int y[kColRuns];
  int len[kColRuns];
  int nRuns;
};


struct YArgs {
  int ncols;     // columns of the [z][column][y] intermediate (its row count per plane)
  int colBegin;  // column range processed: [colBegin, colEnd) (exchange pipelining chunks)
  int colEnd;
  int L;       // end of the plane range processed (exclusive; = local planes)
  int zBegin;  // first plane of the range (plane chunking)
  int n;  // dimY
  int colOfX0;  // column needing the x=0 plane hermitian fill, -1 for none
  long long interStride;  // row stride of the [z][column][y] intermediate (>= n)
  // row (z, column c) of the intermediate starts at z * interZStride + c * interStride
  long long interZStride;
  const int* colOffsets;
  const int* colY;
  const long long* colBase;
  // optional per-column run descriptors (all columns qualify) and their stride
  const ColDesc* colDesc;
  long long colStride;
  int plainSticks;  // backward: stick loads with the default cache policy (see GpuExecutor)
  BatchPtrs batch;
};

struct XArgs {
  int L;       // end of the plane range (exclusive)
  int zBegin;  // first plane of the range
  int Y;
  int n;      // dimX
  int nFreq;  // dimX/2+1 for R2C, dimX for C2C
  int ncols;
  long long interStride;  // row stride of the [z][column][y] intermediate (>= Y)
  long long interZStride;  // as YArgs
  const int* colX;
  const int* xToCol;  // nFreq entries: x -> column or -1 (long-line x stage)
  BatchPtrs batch;
};

// Offset of column c's row inside one plane of the intermediate (a plane holds
// ncols * interStride < 2^31 elements: 32-bit arithmetic per lane).
template <class A>
__host__ __device__ inline int inter_row(const A& a, int c) {
  return c * static_cast<int>(a.interStride);
}

// grid z extent of a launch (1 when unbatched)
inline unsigned batch_dim(const BatchPtrs& b) { return b.count > 1 ? static_cast<unsigned>(b.count) : 1u; }

// Engine geometry for diagnostics (SPFFT_LOG).
std::string describe_engine(int n, bool dbl, bool lineFast);

// Host launchers. `tw` is the length-n twiddle table exp(-2 pi i m / n).
// BT is the exchange element type (cx<T> or cx<float> for *_FLOAT exchanges).
template <typename T, typename BT>
void launch_z_backward(const ZArgs& a, const cx<T>* values, BT* out, const cx<T>* tw,
                       hipStream_t stream);
template <typename T, typename BT>
void launch_z_forward(const ZArgs& a, const BT* in, cx<T>* values, T scale, const cx<T>* tw,
                      hipStream_t stream);
// Fused reciprocal-space operator z stage, in place on the stick side (simple
// sticks: ZArgs::desc non-null): forward z FFT, values[i] = scale * coefficient
// (when `values` is non-null), coefficient *= kernel[i] on the sparse set and
// zero elsewhere, hermitian fill of the (0,0) stick, inverse z FFT. `kernel`
// has one entry per value, real or (complexKernel) interleaved complex.
template <typename T>
void launch_z_reciprocal(const ZArgs& a, cx<T>* sticks, const T* kernel, bool complexKernel,
                         cx<T>* values, T scale, const cx<T>* tw, hipStream_t stream);
// out[i] = in[i] * kernel[i] over sparse values (composed path; out may be in).
template <typename T>
void launch_values_scale(cx<T>* out, const cx<T>* in, const T* kernel, bool complexKernel, long long count,
                         hipStream_t stream);
template <typename T, typename BT>
void launch_y_backward(const YArgs& a, const BT* in, cx<T>* inter, const cx<T>* tw,
                       hipStream_t stream);
template <typename T, typename BT>
void launch_y_forward(const YArgs& a, const cx<T>* inter, BT* out, const cx<T>* tw,
                      hipStream_t stream);
// twHalf: length-n/2 twiddles; when given (R2C, even n) the packed-real
// half-length kernels run instead of the hermitian-extended complex FFT.
template <typename T>
void launch_x_backward(const XArgs& a, bool r2c, const cx<T>* inter, void* space, const cx<T>* tw,
                       const cx<T>* twHalf, hipStream_t stream);
template <typename T>
void launch_x_forward(const XArgs& a, bool r2c, const void* space, cx<T>* inter, const cx<T>* tw,
                      const cx<T>* twHalf, hipStream_t stream);
// Fused local-operator x stage of C2C transforms, in place on the intermediate:
// inverse x FFT, multiply by the real potential [z][y][x] (rows as the space
// domain's), forward x FFT. Batched launches take the potentials from
// XArgs::batch.in and the intermediates from XArgs::batch.out. plainPotential:
// default-policy loads of the potential (one potential shared by a batch)
// instead of streaming ones.
template <typename T>
void launch_x_apply(const XArgs& a, const T* potential, cx<T>* inter, bool plainPotential,
                    const cx<T>* tw, hipStream_t stream);
// In-place multiply of a space domain by a real potential (unfused path).
template <typename T>
void launch_space_scale(void* space, const T* potential, long long count, bool realSpace,
                        hipStream_t stream);

// Fused density x stage of C2C transforms: density[z][y][x] += weights[m] *
// |inverse x FFT of band m's intermediate|^2. Unbatched: one band (`inter`,
// weights[0]). Batched launches take the bands' intermediates from
// XArgs::batch.in and batch.count weights; the bands share `density`, so every
// workgroup loops over them for its tile (the grid is the unbatched grid).
template <typename T>
void launch_x_density(const XArgs& a, const cx<T>* inter, T* density, const T* weights,
                      const cx<T>* tw, hipStream_t stream);
// density[i] += weight * |space[i]|^2 in one pass (composed path).
template <typename T>
void launch_space_density(const void* space, T* density, T weight, long long count, bool realSpace,
                          hipStream_t stream);

// Fused packed-real x stages of R2C transforms with even n whose half-length
// n / 2 has a compile-time engine (x_r2c_fused_fits; the launchers throw
// otherwise): launch_x_apply and launch_x_density on the rows y[m] = s[2m] +
// i s[2m+1] of the packed-real stage, in place on the intermediate, the real
// space domain neither read nor written. `tw` / `twHalf` as launch_x_backward.
// The potential and the density are read and written as pairs (s[2m], s[2m+1]):
// their pointers must be aligned to 2 * sizeof(T). Batched launches as their
// C2C counterparts.
template <typename T>
bool x_r2c_fused_fits(int n);
template <typename T>
void launch_x_apply_r2c(const XArgs& a, const T* potential, cx<T>* inter, bool plainPotential,
                        const cx<T>* tw, const cx<T>* twHalf, hipStream_t stream);
template <typename T>
void launch_x_density_r2c(const XArgs& a, const cx<T>* inter, T* density, const T* weights, const cx<T>* tw,
                          const cx<T>* twHalf, hipStream_t stream);

// Exchange (Fock) pair operator, fused x stages of C2C transforms. Forward: the
// x stage of forward_xy whose rows are conj(a) * b of two space-domain arrays
// [z][y][x]. Backward: the x stage of backward_xy whose result u is not stored:
// acc[z][y][x] += weight * a[z][y][x] * u[z][y][x].
template <typename T>
void launch_x_forward_pair(const XArgs& a, const cx<T>* pa, const cx<T>* pb, cx<T>* inter, const cx<T>* tw,
                           hipStream_t stream);
template <typename T>
void launch_x_backward_fock(const XArgs& a, const cx<T>* inter, const cx<T>* pa, cx<T>* acc, T weight,
                            const cx<T>* tw, hipStream_t stream);
// Batched pair operator (multi_transform_accumulate_fock), one launch per stage
// for batch.count members with identical plans. Forward x: member m's a is
// XArgs::batch.in[m], its b is pb[m], its intermediate batch.out[m]. z stage:
// member m's stick array (in place) is ZArgs::batch.out[m], its kernel K
// batch.in[m]; no values output. Backward x: the members share acc, so every
// workgroup loops over them for its tile, in member order (intermediates
// batch.in[m], pa[m], weights[m]; the grid is the unbatched grid).
template <typename T>
void launch_x_forward_pair_batch(const XArgs& a, const cx<T>* const* pb, bool plainLoads, const cx<T>* tw,
                                 hipStream_t stream);
template <typename T>
void launch_z_reciprocal_batch(const ZArgs& a, bool complexKernel, T scale, const cx<T>* tw, hipStream_t stream);
template <typename T>
void launch_x_backward_fock_batch(const XArgs& a, const cx<T>* const* pa, const T* weights, cx<T>* acc,
                                  const cx<T>* tw, hipStream_t stream);
// Pair operator on the packed-real rows of R2C transforms with even n whose
// half-length n / 2 has a compile-time engine (x_r2c_fock_fits; the launchers
// throw otherwise): a, b and acc are real arrays [z][y][x], read and written as
// pairs (s[2m], s[2m+1]), so their pointers must be aligned to 2 * sizeof(T).
// Forward: the packed-real x stage of forward_xy whose rows are a * b. Backward:
// the packed-real x stage of backward_xy whose result u is not stored: acc +=
// weight * a * u. `tw` / `twHalf` as launch_x_backward. The batched launches as
// their C2C counterparts (batch.in[m] of the forward launch is member m's a).
template <typename T>
bool x_r2c_fock_fits(int n);
template <typename T>
void launch_x_forward_pair_r2c(const XArgs& a, const T* pa, const T* pb, cx<T>* inter, const cx<T>* tw,
                               const cx<T>* twHalf, hipStream_t stream);
template <typename T>
void launch_x_backward_fock_r2c(const XArgs& a, const cx<T>* inter, const T* pa, T* acc, T weight, const cx<T>* tw,
                                const cx<T>* twHalf, hipStream_t stream);
template <typename T>
void launch_x_forward_pair_r2c_batch(const XArgs& a, const T* const* pb, bool plainLoads, const cx<T>* tw,
                                     const cx<T>* twHalf, hipStream_t stream);
template <typename T>
void launch_x_backward_fock_r2c_batch(const XArgs& a, const T* const* pa, const T* weights, T* acc,
                                      const cx<T>* tw, const cx<T>* twHalf, hipStream_t stream);
// Reciprocal fan-out and fan-in z stages (multi_transform_reciprocal_fan_out /
// fan_in, simple sticks, batch.count members with identical plans; member m's
// stick array is ZArgs::batch.out[m], its kernel K batch.in[m]). One workgroup
// per stick block loops over the members (the grid of launch_z_reciprocal).
// Fan-out: c = scale * forward z FFT of member 0's sticks (stored to `values`
// when non-null), then per member the inverse z FFT of K_m * c into its stick
// array, member 0 (in place) last. Fan-in: the sum over the members, in order,
// of K_m * scale * forward z FFT of their sticks, one inverse z FFT into member
// 0's stick array. Both keep the coefficients (their sum) in a second LDS
// region; z_reciprocal_fan_fits tells whether the launch fits the LDS of a
// workgroup (the launchers throw otherwise).
template <typename T>
bool z_reciprocal_fan_fits(const ZArgs& a);
template <typename T>
void launch_z_reciprocal_fan_out(const ZArgs& a, bool complexKernel, cx<T>* values, T scale, const cx<T>* tw,
                                 hipStream_t stream);
template <typename T>
void launch_z_reciprocal_fan_in(const ZArgs& a, bool complexKernel, T scale, const cx<T>* tw, hipStream_t stream);
// acc[i] += in[i] * kernel[i] over sparse values (composed fan-in path).
template <typename T>
void launch_values_scale_add(cx<T>* acc, const cx<T>* in, const T* kernel, bool complexKernel, long long count,
                             hipStream_t stream);
// Value fan-out and fan-in z stages (multi_transform_accumulate_density_fan /
// multi_transform_apply_local_fan; simple sticks, C2C, batch.count members with
// identical plans; member m's stick array is ZArgs::batch.out[m], its kernel
// batch.in[m], null for the identity). Fan-out: per member the inverse z FFT of
// K_m * values into its stick array, the members spread over the grid like a
// batched backward z stage (the LDS of that stage; every member's workgroups
// read the values). Fan-in: one workgroup per stick block loops over the
// members: the sum, in order, of L_m * scale * forward z FFT of their sticks,
// stored once to `output`; the sum lives in a second LDS region, so the launch
// needs z_reciprocal_fan_fits (the launcher throws otherwise).
template <typename T>
void launch_z_values_fan_out(const ZArgs& a, bool complexKernel, const cx<T>* values, const cx<T>* tw,
                             hipStream_t stream);
template <typename T>
void launch_z_values_fan_in(const ZArgs& a, bool complexKernel, cx<T>* output, T scale, const cx<T>* tw,
                            hipStream_t stream);
// acc[i] += in[i] over sparse values (composed value fan, identity kernel).
template <typename T>
void launch_values_add(cx<T>* acc, const cx<T>* in, long long count, hipStream_t stream);
// Spinor operators (multi_transform_apply_local_spinor / accumulate_spin_density):
// x stages of C2C plans that keep the rows of both components (up, down) of a
// tile in LDS, in two regions of the engine's whole line LDS each.
// x_spinor_fits: both regions and the x -> column table fit a workgroup's LDS
// (the launchers throw otherwise); the engines that already take more than
// half of it (the 1024-long shapes; the 512-long ones take 70 KB and fit) do not.
// `potential` and `density` are four real arrays [localZ][Y][X]:
// {v_uu, v_dd, v_ud_re, v_ud_im} and {n_uu, n_dd, n_ud_re, n_ud_im}.
// Apply: in place on the intermediates up[s], dn[s] of `spinors` spinors
// (blockIdx.z = spinor): inverse x FFTs, the 2x2 mix, forward x FFTs.
// plainPotential: default-policy loads (a batch shares the potential).
// Density: density += weights[s] * {|u|^2, |d|^2, u conj(d)} of the inverse x
// FFTs; every workgroup loops over the spinors for its tile, in order.
constexpr int kMaxSpinors = kMaxBatch / 2;
template <typename T>
bool x_spinor_fits(int n);
template <typename T>
void launch_x_spinor_apply(const XArgs& a, int spinors, cx<T>* const* up, cx<T>* const* dn,
                           const T* const* potential, bool plainPotential, const cx<T>* tw,
                           hipStream_t stream);
template <typename T>
void launch_x_spinor_density(const XArgs& a, int spinors, const cx<T>* const* up, const cx<T>* const* dn,
                             const T* weights, T* const* density, const cx<T>* tw, hipStream_t stream);
// Composed spinor paths, one pass over two complex space domains of `count`
// elements: the in-place 2x2 mix, and the four-array density update.
template <typename T>
void launch_space_spinor_mix(cx<T>* up, cx<T>* dn, const T* const* potential, long long count,
                             hipStream_t stream);
template <typename T>
void launch_space_spin_density(const cx<T>* up, const cx<T>* dn, T* const* density, T weight, long long count,
                               hipStream_t stream);
// Composed path, one pass each: space[i] = conj(a[i]) * b[i] and acc[i] +=
// weight * a[i] * space[i] (interleaved complex or, realSpace, real arrays).
template <typename T>
void launch_space_pair(void* space, const T* pa, const T* pb, long long count, bool realSpace,
                       hipStream_t stream);
template <typename T>
void launch_space_fock(const void* space, const T* pa, T* acc, T weight, long long count, bool realSpace,
                       hipStream_t stream);

// Largest run-time FFT length supported in one workgroup (LDS-resident).
int max_device_fft_length(bool doublePrecision);
// true if n has a compile-time (register-resident) kernel: the powers of two
// 16..1024 (FftCT) and the mixed-radix lengths of SPFFT_MR_SIZES (FftMR).
bool has_ct_kernel(int n);

// Non-power-of-two lengths with compile-time mixed-radix kernels (X-macro;
// user configuration: a build may list other lengths, or none, with
// -DSPFFT_MR_SIZES(X)=..., trading compile time for run-time engines).
#ifndef SPFFT_MR_SIZES
#define SPFFT_MR_SIZES(X)                                                                 \
  X(48) X(60) X(72) X(80) X(90) X(96) X(100) X(108) X(120) X(125) X(135) X(144) X(150) X(160) \
  X(180) X(192) X(200) X(216) \
  X(240) X(288) X(320) X(360) X(384) \
  X(400) X(480)
#endif

}  // namespace dev
}  // namespace spfft
