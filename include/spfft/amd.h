/*
 * SpFFT-AMD C extensions (not part of the SpFFT reference API):
 *  - communicators that do not need MPI (callbacks, in-process local group),
 *  - distributed grids over such communicators,
 *  - explicit HIP streams / asynchronous execution, step-wise execution,
 *  - timing report (host timer tree, JSON) and last-error text.
 */
#ifndef SPFFT_AMD_H
#define SPFFT_AMD_H

#include <stddef.h>

#include "spfft/config.h"
#include "spfft/errors.h"
#include "spfft/grid.h"
#include "spfft/grid_float.h"
#include "spfft/transform.h"
#include "spfft/transform_float.h"
#include "spfft/types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef void* SpfftAmdComm;

/* A communicator implemented by the caller. Each function returns 0 on success.
 *  allgather: every rank contributes `bytes`; recv holds size*bytes in rank order.
 *  alltoallv: host buffers, counts and displacements in bytes (size entries each).
 *  destroy:   optional, called once when the last user of the communicator is gone. */
typedef struct SpfftAmdCommCallbacks {
  void* context;
  int rank;
  int size;
  int (*allgather)(void* context, const void* send, void* recv, size_t bytes);
  int (*alltoallv)(void* context, const void* send, const size_t* sendCounts,
                   const size_t* sendDispls, void* recv, const size_t* recvCounts,
                   const size_t* recvDispls);
  int (*barrier)(void* context);
  void (*destroy)(void* context);
} SpfftAmdCommCallbacks;

SPFFT_EXPORT SpfftError spfft_amd_comm_create_callbacks(SpfftAmdComm* comm,
                                                        const SpfftAmdCommCallbacks* callbacks);
/* Creates `size` communicators of one in-process group (comms[r] has rank r). */
SPFFT_EXPORT SpfftError spfft_amd_comm_create_local_group(int size, SpfftAmdComm* comms);
SPFFT_EXPORT SpfftError spfft_amd_comm_destroy(SpfftAmdComm comm);
SPFFT_EXPORT SpfftError spfft_amd_comm_rank(SpfftAmdComm comm, int* rank);
SPFFT_EXPORT SpfftError spfft_amd_comm_size(SpfftAmdComm comm, int* size);
SPFFT_EXPORT SpfftError spfft_amd_grid_create_distributed(
    SpfftGrid* grid, int maxDimX, int maxDimY, int maxDimZ, int maxNumLocalZColumns,
    int maxLocalZLength, SpfftProcessingUnitType processingUnit, int maxNumThreads,
    SpfftAmdComm comm, SpfftExchangeType exchangeType);
SPFFT_EXPORT SpfftError spfft_amd_float_grid_create_distributed(
    SpfftFloatGrid* grid, int maxDimX, int maxDimY, int maxDimZ, int maxNumLocalZColumns,
    int maxLocalZLength, SpfftProcessingUnitType processingUnit, int maxNumThreads,
    SpfftAmdComm comm, SpfftExchangeType exchangeType);
SPFFT_EXPORT SpfftError spfft_amd_grid_exchange_type(SpfftGrid grid, SpfftExchangeType* type);
/* GPU data plane of a distributed grid: "rccl", "ipc" (peer writes across
 * processes), "peer" (peer writes inside a local group), "loopback",
 * "rccl-self" (local group moved by RCCL), or "none" (local or host-only
 * grid). Collective on first call (creates the data plane). */
SPFFT_EXPORT SpfftError spfft_amd_grid_data_plane(SpfftGrid grid, const char** name);
SPFFT_EXPORT SpfftError spfft_amd_float_grid_data_plane(SpfftFloatGrid grid, const char** name);
/* The data plane's setup facts as a JSON object ("kind"; "self_test",
 * "self_test_ms", "devices", "link_GBps_measured", "channel_priority" where they
 * apply). The string
 * stays valid until the calling thread's next call of this function.
 * Collective on first call. */
SPFFT_EXPORT SpfftError spfft_amd_grid_data_plane_info(SpfftGrid grid, const char** json);
SPFFT_EXPORT SpfftError spfft_amd_float_grid_data_plane_info(SpfftFloatGrid grid, const char** json);
/* Device memory a grid allocated (exchange buffers, intermediate, space domain). */
SPFFT_EXPORT SpfftError spfft_amd_grid_device_bytes(SpfftGrid grid, unsigned long long* bytes);
SPFFT_EXPORT SpfftError spfft_amd_float_grid_device_bytes(SpfftFloatGrid grid,
                                                          unsigned long long* bytes);
/* Number of RCCL communicators this process has created. Grids whose
 * communicators have the same members on the same devices share one
 * (SPFFT_RCCL_SHARE=0: one per grid). */
SPFFT_EXPORT SpfftError spfft_amd_rccl_communicators(int* count);
/* HIP streams the library currently owns: private transform streams (created
 * on a transform's first call unless it was given a stream before) and RCCL
 * channel streams (one per shared communicator). */
SPFFT_EXPORT SpfftError spfft_amd_library_streams(int* count);
/* Exchange plan of a GPU transform: plane chunks K and stick blocks I of the
 * pipelined all-to-all (1 and 1: one exchange per direction), whether the
 * stage kernels write into the peers directly (UNBUFFERED / IPC plane), and
 * the number of idle GPUs the exchange relays through (relay plane). Host
 * transforms report zeros. */
SPFFT_EXPORT SpfftError spfft_amd_transform_exchange_plan(SpfftTransform transform, int* chunks,
                                                          int* stickBlocks, int* peerWrites,
                                                          int* relays);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_exchange_plan(SpfftFloatTransform transform,
                                                                int* chunks, int* stickBlocks,
                                                                int* peerWrites, int* relays);
SPFFT_EXPORT SpfftError spfft_amd_float_grid_exchange_type(SpfftFloatGrid grid,
                                                           SpfftExchangeType* type);

/* Execute on `hipStream` (hipStream_t, NULL = legacy default stream).
 * synchronous = 0: return after enqueue. reset_stream: back to the private stream. */
SPFFT_EXPORT SpfftError spfft_amd_transform_set_stream(SpfftTransform transform, void* hipStream,
                                                       int synchronous);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_set_stream(SpfftFloatTransform transform,
                                                             void* hipStream, int synchronous);
SPFFT_EXPORT SpfftError spfft_amd_transform_reset_stream(SpfftTransform transform);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_reset_stream(SpfftFloatTransform transform);
SPFFT_EXPORT SpfftError spfft_amd_transform_synchronize(SpfftTransform transform);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_synchronize(SpfftFloatTransform transform);
SPFFT_EXPORT SpfftError spfft_amd_transform_local_z_offset_rank(SpfftTransform transform, int rank,
                                                                int* offset, int* length);

/* Zero-copy DLPack export (DLManagedTensor*) of the space domain [localZ][Y][X];
 * the tensor keeps the transform and its grid alive until its deleter runs. */
SPFFT_EXPORT SpfftError spfft_amd_transform_space_domain_dlpack(SpfftTransform transform,
                                                                SpfftProcessingUnitType location,
                                                                void** managedTensor);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_space_domain_dlpack(
    SpfftFloatTransform transform, SpfftProcessingUnitType location, void** managedTensor);

/* Step-wise execution (forward: xy, exchange, z; backward: z, exchange, xy). */
SPFFT_EXPORT SpfftError spfft_amd_transform_forward_xy(SpfftTransform t,
                                                       SpfftProcessingUnitType inputLocation);
SPFFT_EXPORT SpfftError spfft_amd_transform_forward_exchange(SpfftTransform t, int nonBlocking);
SPFFT_EXPORT SpfftError spfft_amd_transform_forward_z(SpfftTransform t, double* output,
                                                      SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_transform_backward_z(SpfftTransform t, const double* input);
SPFFT_EXPORT SpfftError spfft_amd_transform_backward_exchange(SpfftTransform t, int nonBlocking);
SPFFT_EXPORT SpfftError spfft_amd_transform_backward_xy(SpfftTransform t,
                                                        SpfftProcessingUnitType outputLocation);
/* The same steps for single precision transforms. */
SPFFT_EXPORT SpfftError spfft_amd_float_transform_forward_xy(SpfftFloatTransform t,
                                                             SpfftProcessingUnitType inputLocation);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_forward_exchange(SpfftFloatTransform t, int nonBlocking);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_forward_z(SpfftFloatTransform t, float* output,
                                                            SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_backward_z(SpfftFloatTransform t, const float* input);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_backward_exchange(SpfftFloatTransform t, int nonBlocking);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_backward_xy(SpfftFloatTransform t,
                                                              SpfftProcessingUnitType outputLocation);

/* Local operator: output = forward(V * backward(input)) in one call, with the
 * real potential V over the local space domain [localZ][dimY][dimX] (double or
 * float as the transform). input, potential and output are host or device
 * pointers (device pointers are used in place, as backward does for its input);
 * input == output is allowed. After the call the contents of the space domain
 * are unspecified: fused plans never form it and leave it untouched, other
 * plans pass through it. Fused are C2C transforms whose x lines fit one
 * workgroup, and R2C transforms with even dimX whose half-length dimX / 2 has a
 * compile-time kernel (the powers of two 16..1024 and the mixed-radix lengths
 * of the build; SPFFT_R2C_FUSE=0 or SPFFT_R2C_PACKED=0 at creation keeps them
 * composed). Odd dimX, other half-lengths, long x lines and host transforms run
 * composed. On a fused R2C plan the potential is read as pairs of elements: a
 * call whose potential is not aligned to 2 * sizeof(element) runs composed. A
 * null potential is SPFFT_INVALID_PARAMETER_ERROR, except on a
 * rank without local planes, whose space domain is empty. */
SPFFT_EXPORT SpfftError spfft_amd_transform_apply_local(SpfftTransform t, const double* input,
                                                        const double* potential, double* output,
                                                        SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_apply_local(SpfftFloatTransform t,
                                                              const float* input,
                                                              const float* potential, float* output,
                                                              SpfftScalingType scaling);
/* *fused = 1 if the plan runs the fused x apply stage on the GPU (C2C, or the
 * packed-real stage of the R2C plans named above), else 0. */
SPFFT_EXPORT SpfftError spfft_amd_transform_apply_local_fused(SpfftTransform t, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_apply_local_fused(SpfftFloatTransform t,
                                                                    int* fused);
/* apply_local of n transforms (distinct grids) with their phases interleaved;
 * identical fused plans on one GPU share one launch per stage (SPFFT_BATCH). */
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_apply_local(int n, SpfftTransform* transforms,
                                                              const double* const* inputs,
                                                              const double* const* potentials,
                                                              double* const* outputs,
                                                              const SpfftScalingType* scalings);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_apply_local(
    int n, SpfftFloatTransform* transforms, const float* const* inputs,
    const float* const* potentials, float* const* outputs, const SpfftScalingType* scalings);

/* Density accumulation: density[z][y][x] += weight * |backward(input)[z][y][x]|^2
 * in one call, with the real array density over the local space domain
 * [localZ][dimY][dimX] (double or float as the transform; for R2C the space
 * value is real and the contribution weight * s^2). density is a host or device
 * pointer, is updated in place and is never zeroed by the library; input is not
 * modified. After the call the contents of the space domain are unspecified:
 * fused plans never form it and leave it untouched, other plans pass through
 * it; which plans are fused is as for spfft_amd_transform_apply_local (C2C with
 * x lines of one workgroup; R2C with even dimX and a compile-time half-length
 * kernel). On a fused R2C plan density is updated as pairs of elements: a call
 * whose density is not aligned to 2 * sizeof(element) runs composed. A
 * null density with local planes is SPFFT_INVALID_PARAMETER_ERROR. */
SPFFT_EXPORT SpfftError spfft_amd_transform_accumulate_density(SpfftTransform t,
                                                               const double* input, double weight,
                                                               double* density);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_accumulate_density(SpfftFloatTransform t,
                                                                     const float* input,
                                                                     float weight, float* density);
/* *fused = 1 if the plan runs the fused x density stage on the GPU (C2C, or the
 * packed-real stage of the R2C plans named above), else 0. */
SPFFT_EXPORT SpfftError spfft_amd_transform_density_fused(SpfftTransform t, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_density_fused(SpfftFloatTransform t, int* fused);
/* density += sum_i weights[i] * |backward_i(inputs[i])|^2 of n transforms
 * (distinct grids, equal space domains) into one shared density, with their
 * phases interleaved; identical fused plans on one GPU share one launch per
 * stage (SPFFT_BATCH). The sum runs in list order: the same call on the same
 * data gives the same bits. */
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_accumulate_density(int n,
                                                                     SpfftTransform* transforms,
                                                                     const double* const* inputs,
                                                                     const double* weights,
                                                                     double* density);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_accumulate_density(
    int n, SpfftFloatTransform* transforms, const float* const* inputs, const float* weights,
    float* density);

/* Reciprocal-space operator: the space domain f of the transform is replaced by
 * backward(K * (scale * forward(f))) in one call, exactly what forward(location,
 * values, scaling), values[i] *= K[i], backward(values, location) give.
 * kernel holds one entry per local frequency value, in the order of the index
 * triplets given at transform creation (the order of forward's output): real
 * (kernelIsComplex = 0) or interleaved complex (kernelIsComplex != 0), double or
 * float as the transform. values may be NULL; otherwise it receives the scaled
 * forward values before the multiply (interleaved complex, as forward's
 * output). kernel and values are host or device pointers. location is where the
 * space domain is read and where the result is written, as in forward and
 * backward. scaling is SPFFT_NO_SCALING or SPFFT_FULL_SCALING. Fused plans (GPU
 * transforms with simple sticks whose z lines fit one workgroup, local or on an
 * exchange other than *_FLOAT without peer writes) run both z FFTs and the
 * multiply in one kernel, without a round trip of the values through memory;
 * other plans run the composition. A null kernel with local elements is
 * SPFFT_INVALID_PARAMETER_ERROR; the transform stays usable after an error. */
SPFFT_EXPORT SpfftError spfft_amd_transform_apply_reciprocal(SpfftTransform t,
                                                             SpfftProcessingUnitType location,
                                                             const double* kernel,
                                                             int kernelIsComplex, double* values,
                                                             SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_apply_reciprocal(SpfftFloatTransform t,
                                                                   SpfftProcessingUnitType location,
                                                                   const float* kernel,
                                                                   int kernelIsComplex, float* values,
                                                                   SpfftScalingType scaling);
/* *fused = 1 if the plan runs the fused z stage on the GPU, else 0. */
SPFFT_EXPORT SpfftError spfft_amd_transform_reciprocal_fused(SpfftTransform t, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_reciprocal_fused(SpfftFloatTransform t, int* fused);

/* Exchange (Fock) pair operator of hybrid functionals in one call:
 *   acc += weight * a * backward(K * (scale * forward(conj(a) * b)))
 * a, b and acc cover the local space domain [localZ][dimY][dimX]: interleaved
 * complex for C2C transforms, real for R2C (conj is then the identity and the
 * update is real); double or float as the transform. kernel (one real or
 * interleaved complex entry per local frequency value) and values (NULL, or the
 * scaled forward values c(G) before the multiply) are as in
 * spfft_amd_transform_apply_reciprocal. All pointers are host or device
 * pointers; host arrays of a GPU transform are staged on its stream. a == b is
 * allowed, acc overlapping a or b is undefined; a and b are not modified.
 * scaling is SPFFT_NO_SCALING or SPFFT_FULL_SCALING. After the call the contents
 * of the space domain are unspecified: fused plans form the pair density in the
 * forward x stage's loads and accumulate from the backward x stage's LDS, never
 * form the space domain and leave it untouched; other plans pass through it.
 * Fused are GPU C2C transforms whose x lines fit one workgroup
 * (spfft_amd_transform_fock_fused) and GPU R2C transforms with even dimX whose
 * half-length dimX / 2 has a compile-time kernel, on the packed-real x stages
 * (spfft_amd_transform_fock_r2c_fused; the plans named at
 * spfft_amd_transform_apply_local, SPFFT_R2C_FUSE=0 or SPFFT_R2C_PACKED=0 at
 * creation keeps them composed). Odd dimX, other half-lengths, long x lines and
 * host transforms run composed. On a fused R2C plan a, b and acc are accessed
 * as pairs of elements: where a device array is not aligned to 2 *
 * sizeof(element), the half of the call that uses it (forward: a, b; backward:
 * a, acc) runs composed and passes through the space domain.
 * The z stage is the one of apply_reciprocal. Collective on distributed
 * grids. A null a, b or acc with local planes, or a null kernel with local
 * values, is SPFFT_INVALID_PARAMETER_ERROR; the transform stays usable. */
SPFFT_EXPORT SpfftError spfft_amd_transform_accumulate_fock(SpfftTransform t, const double* a,
                                                            const double* b, const double* kernel,
                                                            int kernelIsComplex, double weight,
                                                            double* acc, double* values,
                                                            SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_accumulate_fock(SpfftFloatTransform t,
                                                                  const float* a, const float* b,
                                                                  const float* kernel,
                                                                  int kernelIsComplex, float weight,
                                                                  float* acc, float* values,
                                                                  SpfftScalingType scaling);
/* acc += sum_i weights[i] * a[i] * backward_i(K_i * (scale * forward_i(conj(a[i]) * b[i])))
 * of n transforms (distinct grids, equal local space domains, all C2C or all
 * R2C) into one shared acc: the pairs of one band of the exchange operator in
 * one call. a[i], b[i] and acc are as in spfft_amd_transform_accumulate_fock;
 * b[i] may be the same array for every i and may be a[i], acc overlapping any
 * a or b is undefined. kernels[i] holds one entry per local value of transform
 * i, all real or all interleaved complex (kernelIsComplex); the pointers may
 * all be equal. One scaling for the call; there is no values output. All
 * pointers are host or device pointers. Identical plans on one GPU with fused
 * x and z stages (C2C, or the packed-real R2C pair stages; an R2C member whose
 * a[i], b[i] or acc is not aligned to 2 * sizeof(element) runs per transform)
 * and device pointers share one launch per stage, and the
 * workgroup that owns a tile of acc adds the members' updates in list order
 * (SPFFT_BATCH); everything else runs per transform with the phases
 * interleaved. Every update of acc is ordered behind the previous one: the sum
 * order is fixed by the call alone, the same call on the same data gives the
 * same bits. Collective on distributed grids (per transform, in list order).
 * A repeated grid, null transforms, a, b, kernels or weights with n > 0, a null
 * acc, a[i] or b[i] with local planes, a null kernels[i] with local values,
 * unequal space domains or a bad scaling is SPFFT_INVALID_PARAMETER_ERROR; the
 * transforms stay usable. n == 0 is a no-op. */
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_accumulate_fock(
    int n, SpfftTransform* transforms, const double* const* a, const double* const* b,
    const double* const* kernels, int kernelIsComplex, const double* weights, double* acc,
    SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_accumulate_fock(
    int n, SpfftFloatTransform* transforms, const float* const* a, const float* const* b,
    const float* const* kernels, int kernelIsComplex, const float* weights, float* acc,
    SpfftScalingType scaling);
/* *fused = 1 if the plan runs the fused C2C pair x stages on the GPU, else 0
 * (0 on every R2C plan: see spfft_amd_transform_fock_r2c_fused). */
SPFFT_EXPORT SpfftError spfft_amd_transform_fock_fused(SpfftTransform t, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_fock_fused(SpfftFloatTransform t, int* fused);
/* *fused = 1 if the plan runs the packed-real pair x stages (GPU R2C, even dimX,
 * compile-time half-length kernel), else 0: C2C, host, odd dimX, run-time
 * half-lengths, long x lines, SPFFT_R2C_FUSE=0 or SPFFT_R2C_PACKED=0 at
 * creation. A null fused is SPFFT_INVALID_PARAMETER_ERROR. */
SPFFT_EXPORT SpfftError spfft_amd_transform_fock_r2c_fused(SpfftTransform t, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_fock_r2c_fused(SpfftFloatTransform t, int* fused);

/* Reciprocal fan-out (gradient-like): one forward transform feeds n backward
 * transforms,
 *   c = scale * forward_0(space_0),  space_i = backward_i(K_i * c), i = 0 .. n-1,
 * on the space domains of n transforms on distinct grids (a transform and its
 * clones) at location; space_0 is both the input and member 0's result. The
 * transforms must have equal dimensions, type, local planes and local element
 * count: values are matched by position. kernels[i] holds one entry per local
 * value in index order, all real or all interleaved complex (kernelIsComplex);
 * the pointers may be equal. values may be NULL; otherwise it receives c, as in
 * spfft_amd_transform_apply_reciprocal. kernels[i] and values are host or
 * device pointers; scaling is SPFFT_NO_SCALING or SPFFT_FULL_SCALING. Identical
 * plans on one GPU with the fused z stage, device pointers, location
 * SPFFT_PU_GPU, n <= 8 and z lines that fit a workgroup's LDS twice
 * (spfft_amd_transform_reciprocal_fan_fused) run x and y forward of member 0,
 * one z kernel that transforms each stick block once and writes n stick arrays,
 * and one batched launch per backward stage (SPFFT_BATCH); everything else runs
 * forward_0 and, per member in list order, a multiply of the values and
 * backward_i. n == 1 is spfft_amd_transform_apply_reciprocal, n == 0 a no-op.
 * Collective on distributed grids (per transform, in list order). A repeated
 * grid, null transforms or kernels with n > 0, a null kernels[i] with local
 * values, unequal transforms or a bad scaling is SPFFT_INVALID_PARAMETER_ERROR;
 * the transforms stay usable after an error. */
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_reciprocal_fan_out(
    int n, SpfftTransform* transforms, SpfftProcessingUnitType location, const double* const* kernels,
    int kernelIsComplex, double* values, SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_reciprocal_fan_out(
    int n, SpfftFloatTransform* transforms, SpfftProcessingUnitType location, const float* const* kernels,
    int kernelIsComplex, float* values, SpfftScalingType scaling);
/* Reciprocal fan-in (divergence-like): n forward transforms feed one backward
 * transform,
 *   space_0 = backward_0(sum_i K_i * (scale * forward_i(space_i))),
 * summed in list order; the space domains of the members i > 0 are left
 * unchanged. Arguments, fused and composed paths and errors as for
 * spfft_amd_multi_transform_reciprocal_fan_out (the fused z kernel sums the
 * members' coefficients per stick block in LDS; the composition runs forward_i
 * and a multiply-add into one values buffer per member, then backward_0); there
 * is no values output. The sum order is fixed by the call alone: the same call
 * on the same data gives the same bits. */
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_reciprocal_fan_in(
    int n, SpfftTransform* transforms, SpfftProcessingUnitType location, const double* const* kernels,
    int kernelIsComplex, SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_reciprocal_fan_in(
    int n, SpfftFloatTransform* transforms, SpfftProcessingUnitType location, const float* const* kernels,
    int kernelIsComplex, SpfftScalingType scaling);
/* *fused = 1 if t and n - 1 clones of it, called with device pointers at
 * SPFFT_PU_GPU, run the fused z kernel of the two calls above (n == 1: that of
 * apply_reciprocal), else 0. */
SPFFT_EXPORT SpfftError spfft_amd_transform_reciprocal_fan_fused(SpfftTransform t, int n, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_reciprocal_fan_fused(SpfftFloatTransform t, int n,
                                                                       int* fused);

/* Value fans: one array of frequency values fans out through n reciprocal-space
 * kernels into n transforms on distinct grids (a transform and its clones), as
 * the kinetic-energy density and the tau-dependent term of a meta-GGA
 * Hamiltonian need. The transforms must have equal dimensions, type, local
 * planes and local element count: values are matched by position.
 *
 * Density fan:
 *   density[z][y][x] += sum_i weights[i] * |backward_i(K_i * input)[z][y][x]|^2
 * Apply-local fan:
 *   output = sum_i L_i * (scale * forward_i(V_i * backward_i(K_i * input)))
 * both in list order. input and output hold one interleaved-complex entry per
 * local frequency value, in index order; input == output is allowed, input is
 * otherwise not modified. kernels / kernelsIn (K_i) and kernelsOut (L_i) hold
 * one entry per local value, all real or all interleaved complex
 * (kernelIsComplex); a NULL entry is the identity; pointers may repeat.
 * potentials[i] is the real potential over the local space domain as in
 * spfft_amd_transform_apply_local; density and weights are as in
 * spfft_amd_multi_transform_accumulate_density (density is never zeroed). All
 * arrays are host or device pointers (weights and the pointer arrays are host
 * arrays). The sum order is fixed by the call alone: the same call on the same
 * data gives the same bits. The space domains are unspecified afterwards.
 *
 * Identical C2C plans on one GPU with simple sticks, fused x stages, device
 * pointers, n <= 8 and z lines that fit a workgroup's LDS twice
 * (spfft_amd_transform_values_fan_fused) run one z kernel that multiplies each
 * stick block's values by K_i per member and writes n stick arrays, the batched y and x
 * launches of the multi-transform calls and, for the apply-local fan, one z
 * kernel that sums the members' L_i-weighted coefficients per stick block and
 * stores the values once (SPFFT_BATCH). Everything else runs, per member in list
 * order, a multiply of the values, spfft_amd_transform_apply_local /
 * accumulate_density and a multiply-add into one buffer. n == 0 is a no-op.
 * Collective on distributed grids (per transform, in list order). A repeated
 * grid, a null pointer array or weights with n > 0, a null input, output or
 * density while local values or planes exist, a null potentials[i] with local
 * planes, unequal transforms or a bad scaling is SPFFT_INVALID_PARAMETER_ERROR;
 * the transforms stay usable after an error. */
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_accumulate_density_fan(
    int n, SpfftTransform* transforms, const double* input, const double* const* kernels,
    int kernelIsComplex, const double* weights, double* density);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_accumulate_density_fan(
    int n, SpfftFloatTransform* transforms, const float* input, const float* const* kernels,
    int kernelIsComplex, const float* weights, float* density);
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_apply_local_fan(
    int n, SpfftTransform* transforms, const double* input, const double* const* kernelsIn,
    const double* const* potentials, const double* const* kernelsOut, int kernelIsComplex, double* output,
    SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_apply_local_fan(
    int n, SpfftFloatTransform* transforms, const float* input, const float* const* kernelsIn,
    const float* const* potentials, const float* const* kernelsOut, int kernelIsComplex, float* output,
    SpfftScalingType scaling);
/* *fused = 1 if t and n - 1 clones of it, called with device pointers, run the
 * fused z fan kernels of the two calls above, else 0. Whether the x stage
 * between them is fused is what spfft_amd_transform_apply_local_fused /
 * density_fused report. */
SPFFT_EXPORT SpfftError spfft_amd_transform_values_fan_fused(SpfftTransform t, int n, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_values_fan_fused(SpfftFloatTransform t, int n, int* fused);

/* Spinor operators (non-collinear magnetism, spin-orbit coupling). A call takes
 * nSpinors two-component spinors as 2 * nSpinors transforms on distinct grids,
 * in the order up_0, dn_0, up_1, dn_1, ... (a transform and its clones). All
 * must be C2C with equal dimensions, local planes and local element count:
 * values are matched by position. inputs and outputs hold 2 * nSpinors
 * pointers in the same order, one interleaved-complex entry per local
 * frequency value each.
 *
 * potential[4] = {v_uu, v_dd, v_ud_re, v_ud_im}: four real arrays over the local
 * space domain [localZ][dimY][dimX], with v_ud = v_ud_re + i * v_ud_im and
 * v_du = conj(v_ud). For V * 1 + B . sigma that is v_uu = V + B_z,
 * v_dd = V - B_z, v_ud_re = B_x, v_ud_im = -B_y.
 *
 * Spinor local operator, per spinor s:
 *   psi_s   = backward_s(in_s)                                     (s = up, dn)
 *   out_up = scale * forward_up(v_uu * psi_up + v_ud * psi_dn)
 *   out_dn = scale * forward_dn(conj(v_ud) * psi_up + v_dd * psi_dn)
 * out == in per member is allowed; inputs are otherwise not modified; the four
 * potential pointers may repeat.
 *
 * Spin density matrix, density[4] = {n_uu, n_dd, n_ud_re, n_ud_im}, four real
 * arrays over the local space domain:
 *   n_uu += sum_s w_s |psi_up|^2,  n_dd += sum_s w_s |psi_dn|^2,
 *   n_ud += sum_s w_s psi_up * conj(psi_dn)        (n_ud = n_ud_re + i * n_ud_im)
 * The sum runs in list order; the library never zeroes the arrays; weights
 * holds nSpinors entries. The four arrays must be distinct (equal pointers are
 * SPFFT_INVALID_PARAMETER_ERROR; partial overlap is undefined). The charge and
 * magnetisation densities are n = n_uu + n_dd, m_z = n_uu - n_dd,
 * m_x = 2 * n_ud_re, m_y = -2 * n_ud_im.
 *
 * Both calls: the same call on the same data gives the same bits; the space
 * domains are unspecified afterwards. All arrays are host or device pointers
 * (weights and the pointer arrays are host arrays).
 *
 * Identical plans on one GPU with fused x stages, device pointers and x lines
 * that fit a workgroup's LDS twice (spfft_amd_transform_spinor_fused) run the
 * batched z and y launches over all members around one x kernel whose
 * workgroups hold both components' rows of a tile in LDS (SPFFT_BATCH), at
 * most 4 spinors per launch: more run in groups of 4 in list order. Everything
 * else (host transforms, host pointers, distributed grids, long x lines) runs
 * per spinor in list order: backward of both members, one pass over the two
 * space domains, and for the operator forward of both; collective per
 * transform in list order on distributed grids. nSpinors == 0 is a no-op. An
 * R2C member, a repeated grid, unequal transforms, a null pointer array or
 * weights with nSpinors > 0, a null input or output with local values, a null
 * potential or density entry with local planes, equal density pointers or a
 * bad scaling is SPFFT_INVALID_PARAMETER_ERROR; the transforms stay usable
 * after an error. */
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_apply_local_spinor(
    int nSpinors, SpfftTransform* transforms, const double* const* inputs,
    const double* const* potential /*4*/, double* const* outputs, SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_apply_local_spinor(
    int nSpinors, SpfftFloatTransform* transforms, const float* const* inputs,
    const float* const* potential /*4*/, float* const* outputs, SpfftScalingType scaling);
SPFFT_EXPORT SpfftError spfft_amd_multi_transform_accumulate_spin_density(
    int nSpinors, SpfftTransform* transforms, const double* const* inputs, const double* weights,
    double* const* density /*4*/);
SPFFT_EXPORT SpfftError spfft_amd_float_multi_transform_accumulate_spin_density(
    int nSpinors, SpfftFloatTransform* transforms, const float* const* inputs, const float* weights,
    float* const* density /*4*/);
/* *fused = 1 if t and a clone of it, called with device pointers, run the fused
 * spinor x kernels of the two calls above, else 0. */
SPFFT_EXPORT SpfftError spfft_amd_transform_spinor_fused(SpfftTransform t, int* fused);
SPFFT_EXPORT SpfftError spfft_amd_float_transform_spinor_fused(SpfftFloatTransform t, int* fused);

/* Timer tree (SPFFT_TIMING=1 or spfft_amd_timing_enable). enable: 0 off, 1 host
 * scopes only (like the reference's timer), 2 host scopes and GPU stage times
 * (a hipEvent per stage boundary, nodes gpu/<direction>/<stage>). */
SPFFT_EXPORT SpfftError spfft_amd_timing_enable(int enable);
SPFFT_EXPORT SpfftError spfft_amd_timing_reset(void);
/* Writes a JSON report into buffer (truncated to size-1); *required = full length + 1. */
SPFFT_EXPORT SpfftError spfft_amd_timing_json(char* buffer, size_t size, size_t* required);
SPFFT_EXPORT SpfftError spfft_amd_timing_print(char* buffer, size_t size, size_t* required);

/* Text of the last error raised in this thread (empty if none). */
SPFFT_EXPORT const char* spfft_amd_last_error_message(void);
/* Number of HIP devices visible (0 when no GPU runtime/device). */
SPFFT_EXPORT int spfft_amd_device_count(void);
/* Library build information ("gfx950", version, ...). */
SPFFT_EXPORT const char* spfft_amd_build_info(void);

#ifdef __cplusplus
}
#endif

#endif
