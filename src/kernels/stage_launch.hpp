// Stage launchers (templates): one workgroup engine per line length, the
// kernel's LDS and grid, and the launch. Explicit instantiations live in one
// translation unit per stage and precision (z/y/x_stage*.hip), so the stage
// kernels compile in parallel.
// The packed-real R2C x stage runs forward on the row-mapped engine (the first
// FFT pass loads the real rows directly) rather than the line-fast one with the
// rows staged through LDS: 58.9 -> 56.8 us at 256^3 (profiles/r2_s1/shape_ab.txt).
#pragma once

#include "kernels/stage_kernels.hpp"

namespace spfft {
namespace dev {


template <typename T, typename BT>
void launch_z_backward(const ZArgs& a, const cx<T>* values, BT* out, const cx<T>* tw,
                       hipStream_t stream) {
  if (a.numSticks <= a.stickBegin) return;
  with_engine<T, +1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    // (plain stick stores only where the executor asks for them: plainSticks)
    const bool plain = a.plainSticks != 0;
    auto k = !a.desc ? z_backward_kernel<E, T, BT>
             : plain ? z_backward_desc_kernel<E, T, BT, true> : z_backward_desc_kernel<E, T, BT, false>;
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.numSticks - a.stickBegin, lines), 1, batch_dim(a.batch)), dim3(threads),
                       ldsTotal, stream, eng, b, values, out, tw);
    gpu_check_launch("z_backward", stream);
  });
}

template <typename T, typename BT>
void launch_z_forward(const ZArgs& a, const BT* in, cx<T>* values, T scale, const cx<T>* tw,
                      hipStream_t stream) {
  if (a.numSticks <= a.stickBegin) return;
  with_engine<T, -1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    auto k = !a.desc ? z_forward_kernel<E, T, BT>
             : a.ntValueStores ? z_forward_desc_kernel<E, T, BT, true> : z_forward_desc_kernel<E, T, BT, false>;
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    prepare_kernel(k, ldsTotal);
    const unsigned nb = static_cast<unsigned>(ceil_div(a.numSticks - a.stickBegin, lines));
    hipLaunchKernelGGL(k, dim3(nb, 1, batch_dim(b.batch)), dim3(threads), ldsTotal, stream, eng, b, in, values,
                       scale, tw);
    gpu_check_launch("z_forward", stream);
  });
}

// Fused reciprocal-space operator z stage (simple sticks, in place on the stick
// side). The forward and the inverse engine share the backward stage's shape
// (forward_twin), so the launch takes the LDS and grid of launch_z_backward.
template <typename T>
void launch_z_reciprocal(const ZArgs& a, cx<T>* sticks, const T* kernel, bool complexKernel,
                         cx<T>* values, T scale, const cx<T>* tw, hipStream_t stream) {
  if (a.numSticks <= a.stickBegin) return;
  with_engine<T, +1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto fwd = forward_twin(eng);
    using E = decltype(eng);
    using F = decltype(fwd);
    const bool plain = a.plainSticks != 0;
    auto k = complexKernel ? (plain ? z_reciprocal_kernel<E, F, T, true, true> : z_reciprocal_kernel<E, F, T, true, false>)
                           : (plain ? z_reciprocal_kernel<E, F, T, false, true> : z_reciprocal_kernel<E, F, T, false, false>);
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.numSticks - a.stickBegin, lines)), dim3(threads), ldsTotal, stream,
                       eng, fwd, b, sticks, kernel, values, scale, tw);
    gpu_check_launch("z_reciprocal", stream);
  });
}

// out[i] = in[i] * kernel[i] over `count` sparse values (composed path; out may be in)
template <typename T>
void launch_values_scale(cx<T>* out, const cx<T>* in, const T* kernel, bool complexKernel, long long count,
                         hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  if (complexKernel)
    hipLaunchKernelGGL((values_scale_kernel<T, true>), dim3(blocks), dim3(256), 0, stream, out, in, kernel, count);
  else
    hipLaunchKernelGGL((values_scale_kernel<T, false>), dim3(blocks), dim3(256), 0, stream, out, in, kernel, count);
  gpu_check_launch("values_scale", stream);
}

template <typename T, typename BT>
void launch_y_backward(const YArgs& a, const BT* in, cx<T>* inter, const cx<T>* tw,
                       hipStream_t stream) {
  if (a.colEnd <= a.colBegin || a.L <= a.zBegin) return;
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto k = a.plainSticks ? y_backward_kernel<decltype(eng), T, BT, true> : y_backward_kernel<decltype(eng), T, BT, false>;
    const std::size_t ldsTotal = lds + col_entries_lds(a, true, y_table<decltype(eng), true>());
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, y_grid(a.colEnd - a.colBegin, ceil_div(a.L - a.zBegin, lines), batch_dim(a.batch)), dim3(threads), ldsTotal, stream, eng, a,
                       in, inter, tw);
    gpu_check_launch("y_backward", stream);
  });
}

template <typename T, typename BT>
void launch_y_forward(const YArgs& a, const cx<T>* inter, BT* out, const cx<T>* tw,
                      hipStream_t stream) {
  if (a.colEnd <= a.colBegin || a.L <= a.zBegin) return;
  with_engine<T, -1, true, !std::is_same<T, float>::value>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto k = y_forward_kernel<decltype(eng), T, BT>;
    const std::size_t ldsTotal = lds + col_entries_lds(a, false, y_table<decltype(eng), has_store_pos<decltype(eng)>::value>());
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, y_grid(a.colEnd - a.colBegin, ceil_div(a.L - a.zBegin, lines), batch_dim(a.batch)), dim3(threads), ldsTotal, stream, eng, a,
                       inter, out, tw);
    gpu_check_launch("y_forward", stream);
  });
}

template <typename T>
void launch_x_backward(const XArgs& a, bool r2c, const cx<T>* inter, void* space,
                       const cx<T>* tw, const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  if (r2c && twHalf && a.n % 2 == 0 && a.n >= 4) {
    with_engine<T, +1, true>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
      auto k = x_backward_c2r_kernel<decltype(eng), T>;
      const std::size_t ldsTotal =
          lds + std::size_t(lines) * sizeof(cx<T>) + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, batch_dim(a.batch)), dim3(threads), ldsTotal,
                         stream, eng, a, inter, static_cast<T*>(space), twHalf, tw);
      gpu_check_launch("x_backward_c2r", stream);
    });
    return;
  }
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto k = r2c ? x_backward_kernel<decltype(eng), T, true> : x_backward_kernel<decltype(eng), T, false>;
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, batch_dim(a.batch)), dim3(threads), ldsTotal, stream, eng, a,
                       inter, space, tw);
    gpu_check_launch("x_backward", stream);
  });
}

template <typename T>
void launch_x_forward(const XArgs& a, bool r2c, const void* space, cx<T>* inter,
                      const cx<T>* tw, const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  if (r2c && twHalf && a.n % 2 == 0 && a.n >= 4) {
    with_engine<T, -1, false>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
      auto k = x_forward_r2c_kernel<decltype(eng), T>;
      const std::size_t ldsTotal = lds + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, batch_dim(a.batch)), dim3(threads), ldsTotal,
                         stream, eng, a, static_cast<const T*>(space), inter, twHalf, tw);
      gpu_check_launch("x_forward_r2c", stream);
    });
    return;
  }
  with_engine<T, -1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto k = r2c ? x_forward_kernel<decltype(eng), T, true> : x_forward_kernel<decltype(eng), T, false>;
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, batch_dim(a.batch)), dim3(threads), ldsTotal, stream, eng, a,
                       space, inter, tw);
    gpu_check_launch("x_forward", stream);
  });
}

// Fused local-operator x stage (C2C, in place on the intermediate). The inverse
// and the forward engine share the backward stage's shape (forward_twin).
template <typename T>
void launch_x_apply(const XArgs& a, const T* potential, cx<T>* inter, bool plainPotential,
                    const cx<T>* tw, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto fwd = forward_twin(eng);
    using E = decltype(eng);
    using F = decltype(fwd);
    auto k = plainPotential ? x_apply_kernel<E, F, T, false> : x_apply_kernel<E, F, T, true>;
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, batch_dim(a.batch)), dim3(threads), ldsTotal, stream, eng, fwd, a,
                       potential, inter, tw);
    gpu_check_launch("x_apply", stream);
  });
}

// space[i] *= potential[i] over `count` elements (complex or, realSpace, real)
template <typename T>
void launch_space_scale(void* space, const T* potential, long long count, bool realSpace,
                        hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  if (realSpace)
    hipLaunchKernelGGL((space_scale_kernel<T, T>), dim3(blocks), dim3(256), 0, stream,
                       static_cast<T*>(space), potential, count);
  else
    hipLaunchKernelGGL((space_scale_kernel<cx<T>, T>), dim3(blocks), dim3(256), 0, stream,
                       static_cast<cx<T>*>(space), potential, count);
  gpu_check_launch("space_scale", stream);
}

// Cache policy of the rho accesses of a single-band x density launch: streaming
// (true) or plain (false); A/B in profiles/r8/density.
#ifndef SPFFT_DENSITY_STREAM_RHO
#define SPFFT_DENSITY_STREAM_RHO 1
#endif

// Fused density x stage (C2C): density += weights[m] |inverse x FFT|^2 over the
// bands m of the launch, which the workgroups loop over (grid as unbatched).
template <typename T>
void launch_x_density(const XArgs& a, const cx<T>* inter, T* density, const T* weights,
                      const cx<T>* tw, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  const int bands = a.batch.count > 1 ? a.batch.count : 1;
  DensityWeights<T> w{};
  for (int m = 0; m < bands && m < kMaxBatch; ++m) w.w[m] = weights[m];
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    const dim3 grid(ceil_div(a.Y, lines), a.L - a.zBegin, 1);
    auto single = x_density_kernel<E, T, SPFFT_DENSITY_STREAM_RHO != 0, false>;
    if constexpr (DensityBandLoop<E>::value) {
      if (bands > 1) {
        // the bands of a batch revisit the tile of rho: default-policy accesses
        auto k = x_density_kernel<E, T, false, true>;
        prepare_kernel(k, ldsTotal);
        hipLaunchKernelGGL(k, grid, dim3(threads), ldsTotal, stream, eng, a, inter, density, w, tw);
        gpu_check_launch("x_density", stream);
        return;
      }
    }
    prepare_kernel(single, ldsTotal);
    XArgs one = a;
    one.batch.count = 0;
    for (int m = 0; m < bands; ++m) {
      DensityWeights<T> wm{};
      wm.w[0] = w.w[m];
      hipLaunchKernelGGL(single, grid, dim3(threads), ldsTotal, stream, eng, one,
                         bands > 1 ? static_cast<const cx<T>*>(a.batch.in[m]) : inter, density, wm, tw);
      gpu_check_launch("x_density", stream);
    }
  });
}

// density[i] += weight |space[i]|^2 over `count` elements (complex or, realSpace, real)
template <typename T>
void launch_space_density(const void* space, T* density, T weight, long long count, bool realSpace,
                          hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  if (realSpace)
    hipLaunchKernelGGL((space_density_kernel<T, T>), dim3(blocks), dim3(256), 0, stream,
                       static_cast<const T*>(space), density, weight, count);
  else
    hipLaunchKernelGGL((space_density_kernel<cx<T>, T>), dim3(blocks), dim3(256), 0, stream,
                       static_cast<const cx<T>*>(space), density, weight, count);
  gpu_check_launch("space_density", stream);
}

// Fused packed-real x stages (R2C, even n, compile-time half-length engine):
// the line-fast backward engine of length n / 2 and the LDS and grid of the C2R
// launch in launch_x_backward. x_r2c_fused_fits tells whether the engine of the
// half-length n / 2 has these kernels (the launchers throw otherwise).
template <typename T>
bool x_r2c_fused_fits(int n) {
  if (n < 4 || n % 2 != 0 || !has_ct_kernel(n / 2)) return false;
  bool fits = false;
  with_engine<T, +1, true>(n / 2, [&](auto eng, int, int, std::size_t) { fits = R2cFuseFits<decltype(eng)>::value; });
  return fits;
}

template <typename T>
void launch_x_apply_r2c(const XArgs& a, const T* potential, cx<T>* inter, bool plainPotential,
                        const cx<T>* tw, const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  if (!twHalf || !has_ct_kernel(a.n / 2)) throw InternalError();
  with_engine<T, +1, true>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (R2cFuseFits<E>::value) {
      auto fwd = forward_twin(eng);
      using F = decltype(fwd);
      auto k = plainPotential ? x_apply_r2c_kernel<E, F, T, false> : x_apply_r2c_kernel<E, F, T, true>;
      const std::size_t ldsTotal =
          lds + std::size_t(lines) * sizeof(cx<T>) + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, batch_dim(a.batch)), dim3(threads), ldsTotal,
                         stream, eng, fwd, a, potential, inter, twHalf, tw);
      gpu_check_launch("x_apply_r2c", stream);
    } else {
      throw InternalError();
    }
  });
}

template <typename T>
void launch_x_density_r2c(const XArgs& a, const cx<T>* inter, T* density, const T* weights, const cx<T>* tw,
                          const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  if (!twHalf || !has_ct_kernel(a.n / 2)) throw InternalError();
  const int bands = a.batch.count > 1 ? a.batch.count : 1;
  DensityWeights<T> w{};
  for (int m = 0; m < bands && m < kMaxBatch; ++m) w.w[m] = weights[m];
  with_engine<T, +1, true>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (R2cFuseFits<E>::value) {
      const std::size_t ldsTotal =
          lds + std::size_t(lines) * sizeof(cx<T>) + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      const dim3 grid(ceil_div(a.Y, lines), a.L - a.zBegin, 1);
      if constexpr (R2cDensityBandLoop<E>::value) {
        if (bands > 1) {
          // the bands of a batch revisit the tile of rho: default-policy accesses
          auto k = x_density_r2c_kernel<E, T, false, true>;
          prepare_kernel(k, ldsTotal);
          hipLaunchKernelGGL(k, grid, dim3(threads), ldsTotal, stream, eng, a, inter, density, w, twHalf, tw);
          gpu_check_launch("x_density_r2c", stream);
          return;
        }
      }
      auto single = x_density_r2c_kernel<E, T, SPFFT_DENSITY_STREAM_RHO != 0, false>;
      prepare_kernel(single, ldsTotal);
      XArgs one = a;
      one.batch.count = 0;
      for (int m = 0; m < bands; ++m) {
        DensityWeights<T> wm{};
        wm.w[0] = w.w[m];
        hipLaunchKernelGGL(single, grid, dim3(threads), ldsTotal, stream, eng, one,
                           bands > 1 ? static_cast<const cx<T>*>(a.batch.in[m]) : inter, density, wm, twHalf, tw);
        gpu_check_launch("x_density_r2c", stream);
      }
    } else {
      throw InternalError();
    }
  });
}

// Cache policy of the fused pair operator's space-array accesses (a, b in the
// forward x stage; a, acc in the backward x stage): streaming (1) or plain (0).
#ifndef SPFFT_FOCK_STREAM
#define SPFFT_FOCK_STREAM 1
#endif

// Forward x stage of the pair density (C2C): rows conj(a) * b, launch geometry
// of launch_x_forward.
template <typename T>
void launch_x_forward_pair(const XArgs& a, const cx<T>* pa, const cx<T>* pb, cx<T>* inter, const cx<T>* tw,
                           hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  with_engine<T, -1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto k = x_forward_pair_kernel<decltype(eng), T, SPFFT_FOCK_STREAM != 0>;
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, 1), dim3(threads), ldsTotal, stream, eng, a,
                       pa, pb, inter, tw);
    gpu_check_launch("x_forward_pair", stream);
  });
}

// Backward x stage of the pair operator (C2C): acc += weight * a * inverse x
// FFT, launch geometry of launch_x_backward.
template <typename T>
void launch_x_backward_fock(const XArgs& a, const cx<T>* inter, const cx<T>* pa, cx<T>* acc, T weight,
                            const cx<T>* tw, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto k = x_backward_fock_kernel<decltype(eng), T, SPFFT_FOCK_STREAM != 0>;
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, 1), dim3(threads), ldsTotal, stream, eng, a,
                       inter, pa, acc, weight, tw);
    gpu_check_launch("x_backward_fock", stream);
  });
}

// Batched pair operator: the members over the grid's z extent in the forward x
// and the z stage, looped over inside the workgroup in the accumulating x stage.
// plainLoads: default-policy loads of a and b (one b shared by the batch: the
// later members find it in the caches) instead of streaming ones.
template <typename T>
void launch_x_forward_pair_batch(const XArgs& a, const cx<T>* const* pb, bool plainLoads, const cx<T>* tw,
                                 hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0 || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  PairSecond<T> second{};
  for (int m = 0; m < a.batch.count; ++m) second.b[m] = pb[m];
  with_engine<T, -1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    auto k = plainLoads ? x_forward_pair_batch_kernel<E, T, false> : x_forward_pair_batch_kernel<E, T, true>;
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, static_cast<unsigned>(a.batch.count)),
                       dim3(threads), ldsTotal, stream, eng, a, second, tw);
    gpu_check_launch("x_forward_pair_batch", stream);
  });
}

template <typename T>
void launch_z_reciprocal_batch(const ZArgs& a, bool complexKernel, T scale, const cx<T>* tw, hipStream_t stream) {
  if (a.numSticks <= a.stickBegin || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  with_engine<T, +1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto fwd = forward_twin(eng);
    using E = decltype(eng);
    using F = decltype(fwd);
    const bool plain = a.plainSticks != 0;
    auto k = complexKernel
                 ? (plain ? z_reciprocal_batch_kernel<E, F, T, true, true> : z_reciprocal_batch_kernel<E, F, T, true, false>)
                 : (plain ? z_reciprocal_batch_kernel<E, F, T, false, true> : z_reciprocal_batch_kernel<E, F, T, false, false>);
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.numSticks - a.stickBegin, lines), 1, static_cast<unsigned>(a.batch.count)),
                       dim3(threads), ldsTotal, stream, eng, fwd, b, scale, tw);
    gpu_check_launch("z_reciprocal_batch", stream);
  });
}

template <typename T>
void launch_x_backward_fock_batch(const XArgs& a, const cx<T>* const* pa, const T* weights, cx<T>* acc,
                                  const cx<T>* tw, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0 || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  FockMembers<T> members{};
  for (int m = 0; m < a.batch.count; ++m) {
    members.a[m] = pa[m];
    members.w[m] = weights[m];
  }
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    const std::size_t ldsTotal = lds + std::size_t(a.n) * sizeof(int) + 16;
    const dim3 grid(ceil_div(a.Y, lines), a.L - a.zBegin, 1);
    if constexpr (FockBandLoop<E>::value) {
      auto k = x_backward_fock_batch_kernel<E, T>;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, grid, dim3(threads), ldsTotal, stream, eng, a, members, acc, tw);
      gpu_check_launch("x_backward_fock_batch", stream);
    } else {
      auto single = x_backward_fock_kernel<E, T, SPFFT_FOCK_STREAM != 0>;
      prepare_kernel(single, ldsTotal);
      XArgs one = a;
      one.batch.count = 0;
      for (int m = 0; m < a.batch.count; ++m) {
        hipLaunchKernelGGL(single, grid, dim3(threads), ldsTotal, stream, eng, one,
                           static_cast<const cx<T>*>(a.batch.in[m]), members.a[m], acc, members.w[m], tw);
        gpu_check_launch("x_backward_fock", stream);
      }
    }
  });
}

// Pair operator on packed-real rows (R2C, even n, compile-time half-length
// engines): the forward launch takes the engine, LDS and grid of the R2C launch
// in launch_x_forward, the accumulating one those of launch_x_density_r2c.
// x_r2c_fock_fits tells whether both engines of the half-length n / 2 have these
// kernels (the launchers throw otherwise).
template <typename T>
bool x_r2c_fock_fits(int n) {
  if (!x_r2c_fused_fits<T>(n)) return false;
  bool fwd = false, bwd = false;
  with_engine<T, -1, false>(n / 2, [&](auto eng, int, int, std::size_t) { fwd = R2cFuseFits<decltype(eng)>::value; });
  with_engine<T, +1, true>(n / 2, [&](auto eng, int, int, std::size_t) { bwd = R2cFuseFits<decltype(eng)>::value; });
  return fwd && bwd;
}

template <typename T>
void launch_x_forward_pair_r2c(const XArgs& a, const T* pa, const T* pb, cx<T>* inter, const cx<T>* tw,
                               const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  if (!twHalf || !has_ct_kernel(a.n / 2)) throw InternalError();
  with_engine<T, -1, false>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (R2cFuseFits<E>::value) {
      auto k = x_forward_pair_r2c_kernel<E, T, SPFFT_FOCK_STREAM != 0>;
      const std::size_t ldsTotal = lds + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, 1), dim3(threads), ldsTotal, stream, eng, a,
                         pa, pb, inter, twHalf, tw);
      gpu_check_launch("x_forward_pair_r2c", stream);
    } else {
      throw InternalError();
    }
  });
}

template <typename T>
void launch_x_backward_fock_r2c(const XArgs& a, const cx<T>* inter, const T* pa, T* acc, T weight, const cx<T>* tw,
                                const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0) return;
  if (!twHalf || !has_ct_kernel(a.n / 2)) throw InternalError();
  with_engine<T, +1, true>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (R2cFuseFits<E>::value) {
      auto k = x_backward_fock_r2c_kernel<E, T, SPFFT_FOCK_STREAM != 0>;
      const std::size_t ldsTotal =
          lds + std::size_t(lines) * sizeof(cx<T>) + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, 1), dim3(threads), ldsTotal, stream, eng, a,
                         inter, pa, acc, weight, twHalf, tw);
      gpu_check_launch("x_backward_fock_r2c", stream);
    } else {
      throw InternalError();
    }
  });
}

template <typename T>
void launch_x_forward_pair_r2c_batch(const XArgs& a, const T* const* pb, bool plainLoads, const cx<T>* tw,
                                     const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0 || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  if (!twHalf || !has_ct_kernel(a.n / 2)) throw InternalError();
  PairSecond<T> second{};
  for (int m = 0; m < a.batch.count; ++m) second.b[m] = reinterpret_cast<const cx<T>*>(pb[m]);
  with_engine<T, -1, false>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (R2cFuseFits<E>::value) {
      auto k = plainLoads ? x_forward_pair_r2c_batch_kernel<E, T, false> : x_forward_pair_r2c_batch_kernel<E, T, true>;
      const std::size_t ldsTotal = lds + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, static_cast<unsigned>(a.batch.count)),
                         dim3(threads), ldsTotal, stream, eng, a, second, twHalf, tw);
      gpu_check_launch("x_forward_pair_r2c_batch", stream);
    } else {
      throw InternalError();
    }
  });
}

template <typename T>
void launch_x_backward_fock_r2c_batch(const XArgs& a, const T* const* pa, const T* weights, T* acc,
                                      const cx<T>* tw, const cx<T>* twHalf, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0 || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  if (!twHalf || !has_ct_kernel(a.n / 2)) throw InternalError();
  FockMembers<T> members{};
  for (int m = 0; m < a.batch.count; ++m) {
    members.a[m] = reinterpret_cast<const cx<T>*>(pa[m]);
    members.w[m] = weights[m];
  }
  with_engine<T, +1, true>(a.n / 2, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (R2cFuseFits<E>::value) {
      const std::size_t ldsTotal =
          lds + std::size_t(lines) * sizeof(cx<T>) + std::size_t(a.n / 2 + 1) * sizeof(int) + 16;
      const dim3 grid(ceil_div(a.Y, lines), a.L - a.zBegin, 1);
      if constexpr (R2cFockBandLoop<E>::value) {
        auto k = x_backward_fock_r2c_batch_kernel<E, T>;
        prepare_kernel(k, ldsTotal);
        hipLaunchKernelGGL(k, grid, dim3(threads), ldsTotal, stream, eng, a, members, acc, twHalf, tw);
        gpu_check_launch("x_backward_fock_r2c_batch", stream);
      } else {
        auto single = x_backward_fock_r2c_kernel<E, T, SPFFT_FOCK_STREAM != 0>;
        prepare_kernel(single, ldsTotal);
        XArgs one = a;
        one.batch.count = 0;
        for (int m = 0; m < a.batch.count; ++m) {
          hipLaunchKernelGGL(single, grid, dim3(threads), ldsTotal, stream, eng, one,
                             static_cast<const cx<T>*>(a.batch.in[m]), pa[m], acc, members.w[m], twHalf, tw);
          gpu_check_launch("x_backward_fock_r2c", stream);
        }
      }
    } else {
      throw InternalError();
    }
  });
}

// space[i] = conj(a[i]) * b[i] over `count` elements (complex or, realSpace, real)
template <typename T>
void launch_space_pair(void* space, const T* pa, const T* pb, long long count, bool realSpace,
                       hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  if (realSpace)
    hipLaunchKernelGGL((space_pair_kernel<T, T>), dim3(blocks), dim3(256), 0, stream, static_cast<T*>(space), pa,
                       pb, count);
  else
    hipLaunchKernelGGL((space_pair_kernel<cx<T>, T>), dim3(blocks), dim3(256), 0, stream,
                       static_cast<cx<T>*>(space), reinterpret_cast<const cx<T>*>(pa),
                       reinterpret_cast<const cx<T>*>(pb), count);
  gpu_check_launch("space_pair", stream);
}

// acc[i] += weight * a[i] * space[i] over `count` elements (complex or, realSpace, real)
template <typename T>
void launch_space_fock(const void* space, const T* pa, T* acc, T weight, long long count, bool realSpace,
                       hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  if (realSpace)
    hipLaunchKernelGGL((space_fock_kernel<T, T>), dim3(blocks), dim3(256), 0, stream,
                       static_cast<const T*>(space), pa, acc, weight, count);
  else
    hipLaunchKernelGGL((space_fock_kernel<cx<T>, T>), dim3(blocks), dim3(256), 0, stream,
                       static_cast<const cx<T>*>(space), reinterpret_cast<const cx<T>*>(pa),
                       reinterpret_cast<cx<T>*>(acc), weight, count);
  gpu_check_launch("space_fock", stream);
}

// Reciprocal fan-out / fan-in z stages: the launch of launch_z_reciprocal (LDS
// and grid of the backward z stage) plus the second LDS region that holds the
// coefficients (fan-out) or their sum (fan-in), lines * n elements behind the
// launch's other LDS. The workgroups loop over the batch.count members.
constexpr std::size_t kFanLdsLimit = 160 * 1024;
// byte offset of the hold region and the launch's LDS bytes
inline std::size_t fan_hold_offset(std::size_t ldsTotal) { return (ldsTotal + 15) / 16 * 16; }
template <typename T>
inline std::size_t fan_lds_bytes(std::size_t ldsTotal, int lines, int n) {
  return fan_hold_offset(ldsTotal) + static_cast<std::size_t>(lines) * n * sizeof(cx<T>);
}

template <typename T>
bool z_reciprocal_fan_fits(const ZArgs& a) {
  std::size_t fft = 0;
  int lines = 0;
  if (has_ct_kernel(a.n)) {
    with_engine<T, +1>(a.n, [&](auto, int, int l, std::size_t lds) {
      lines = l;
      fft = lds;
    });
  } else {
    fft = in_lds_engine_bytes(a.n, sizeof(cx<T>), lines);
  }
  std::size_t ldsTotal = 0;
  z_args_for_lds(a, fft, lines, &ldsTotal);
  return fan_lds_bytes<T>(ldsTotal, lines, a.n) <= kFanLdsLimit;
}

template <typename T>
void launch_z_reciprocal_fan_out(const ZArgs& a, bool complexKernel, cx<T>* values, T scale, const cx<T>* tw,
                                 hipStream_t stream) {
  if (a.numSticks <= a.stickBegin || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  with_engine<T, +1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto fwd = forward_twin(eng);
    using E = decltype(eng);
    using F = decltype(fwd);
    const bool plain = a.plainSticks != 0;
    auto k = complexKernel ? (plain ? z_reciprocal_fan_out_kernel<E, F, T, true, true>
                                    : z_reciprocal_fan_out_kernel<E, F, T, true, false>)
                           : (plain ? z_reciprocal_fan_out_kernel<E, F, T, false, true>
                                    : z_reciprocal_fan_out_kernel<E, F, T, false, false>);
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    const std::size_t bytes = fan_lds_bytes<T>(ldsTotal, lines, a.n);
    if (bytes > kFanLdsLimit) throw InternalError();
    prepare_kernel(k, bytes);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.numSticks - a.stickBegin, lines)), dim3(threads), bytes, stream, eng, fwd,
                       b, values, scale, static_cast<int>(fan_hold_offset(ldsTotal)), tw);
    gpu_check_launch("z_reciprocal_fan_out", stream);
  });
}

template <typename T>
void launch_z_reciprocal_fan_in(const ZArgs& a, bool complexKernel, T scale, const cx<T>* tw, hipStream_t stream) {
  if (a.numSticks <= a.stickBegin || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  with_engine<T, +1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto fwd = forward_twin(eng);
    using E = decltype(eng);
    using F = decltype(fwd);
    const bool plain = a.plainSticks != 0;
    auto k = complexKernel ? (plain ? z_reciprocal_fan_in_kernel<E, F, T, true, true>
                                    : z_reciprocal_fan_in_kernel<E, F, T, true, false>)
                           : (plain ? z_reciprocal_fan_in_kernel<E, F, T, false, true>
                                    : z_reciprocal_fan_in_kernel<E, F, T, false, false>);
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    const std::size_t bytes = fan_lds_bytes<T>(ldsTotal, lines, a.n);
    if (bytes > kFanLdsLimit) throw InternalError();
    prepare_kernel(k, bytes);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.numSticks - a.stickBegin, lines)), dim3(threads), bytes, stream, eng, fwd,
                       b, scale, static_cast<int>(fan_hold_offset(ldsTotal)), tw);
    gpu_check_launch("z_reciprocal_fan_in", stream);
  });
}

// Value fan-out / fan-in z stages. Fan-out: the launch of launch_z_backward
// (its LDS), one grid plane per member (blockIdx.z, also for one member).
// Fan-in: the unbatched grid, the workgroups loop over the batch.count
// members, plus the second LDS region of the reciprocal fans for the sum
// (fan_lds_bytes; z_reciprocal_fan_fits is its fit test).
template <typename T>
void launch_z_values_fan_out(const ZArgs& a, bool complexKernel, const cx<T>* values, const cx<T>* tw,
                             hipStream_t stream) {
  if (a.numSticks <= a.stickBegin || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  if (!a.desc) throw InternalError();
  with_engine<T, +1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    const bool plain = a.plainSticks != 0;
    auto k = complexKernel ? (plain ? z_values_fan_out_kernel<E, T, true, true>
                                    : z_values_fan_out_kernel<E, T, true, false>)
                           : (plain ? z_values_fan_out_kernel<E, T, false, true>
                                    : z_values_fan_out_kernel<E, T, false, false>);
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    prepare_kernel(k, ldsTotal);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.numSticks - a.stickBegin, lines), 1, static_cast<unsigned>(a.batch.count)),
                       dim3(threads), ldsTotal, stream, eng, b, values, tw);
    gpu_check_launch("z_values_fan_out", stream);
  });
}

template <typename T>
void launch_z_values_fan_in(const ZArgs& a, bool complexKernel, cx<T>* output, T scale, const cx<T>* tw,
                            hipStream_t stream) {
  if (a.numSticks <= a.stickBegin || a.batch.count < 1 || a.batch.count > kMaxBatch) return;
  if (!a.desc) throw InternalError();
  with_engine<T, +1>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    auto fwd = forward_twin(eng);
    using E = decltype(eng);
    using F = decltype(fwd);
    auto k = complexKernel ? z_values_fan_in_kernel<E, F, T, true> : z_values_fan_in_kernel<E, F, T, false>;
    std::size_t ldsTotal = 0;
    const ZArgs b = z_args_for_lds(a, lds, lines, &ldsTotal);
    const std::size_t bytes = fan_lds_bytes<T>(ldsTotal, lines, a.n);
    if (bytes > kFanLdsLimit) throw InternalError();
    prepare_kernel(k, bytes);
    hipLaunchKernelGGL(k, dim3(ceil_div(a.numSticks - a.stickBegin, lines)), dim3(threads), bytes, stream, eng, fwd,
                       b, output, scale, static_cast<int>(fan_hold_offset(ldsTotal)), tw);
    gpu_check_launch("z_values_fan_in", stream);
  });
}

// Spinor x stages: the grid of launch_x_apply / launch_x_density, the LDS of
// two line regions and the x -> column table (spinor_lds_bytes). The fit test
// follows z_reciprocal_fan_fits: the engine's LDS without instantiating it.
template <typename T>
bool x_spinor_fits(int n) {
  std::size_t fft = 0;
  int lines = 0;
  if (has_ct_kernel(n)) {
    with_engine<T, +1, true>(n, [&](auto, int, int, std::size_t lds) { fft = lds; });
  } else {
    fft = in_lds_engine_bytes(n, sizeof(cx<T>), lines);
  }
  return spinor_lds_bytes(fft, n) <= kSpinorLdsLimit;
}

template <typename T>
void launch_x_spinor_apply(const XArgs& a, int spinors, cx<T>* const* up, cx<T>* const* dn,
                           const T* const* potential, bool plainPotential, const cx<T>* tw,
                           hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0 || spinors < 1) return;
  if (spinors > kMaxSpinors) throw InternalError();
  SpinorApplyArgs<T> sp{};
  for (int s = 0; s < spinors; ++s) {
    sp.up[s] = up[s];
    sp.dn[s] = dn[s];
  }
  for (int k = 0; k < 4; ++k) sp.v[k] = potential[k];
  XArgs one = a;
  one.batch.count = 0;
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (SpinorFits<E>::value) {
      auto fwd = forward_twin(eng);
      using F = decltype(fwd);
      const std::size_t ldsTotal = spinor_lds_bytes(lds, a.n);
      if (ldsTotal > kSpinorLdsLimit) throw InternalError();
      auto k = plainPotential ? x_spinor_apply_kernel<E, F, T, false> : x_spinor_apply_kernel<E, F, T, true>;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, static_cast<unsigned>(spinors)),
                         dim3(threads), ldsTotal, stream, eng, fwd, one, sp,
                         static_cast<int>(spinor_region_bytes(lds) / sizeof(cx<T>)), tw);
      gpu_check_launch("x_spinor_apply", stream);
    } else {
      throw InternalError();
    }
  });
}

template <typename T>
void launch_x_spinor_density(const XArgs& a, int spinors, const cx<T>* const* up, const cx<T>* const* dn,
                             const T* weights, T* const* density, const cx<T>* tw, hipStream_t stream) {
  if (a.L <= a.zBegin || a.Y <= 0 || spinors < 1) return;
  if (spinors > kMaxSpinors) throw InternalError();
  SpinorDensityArgs<T> sp{};
  for (int s = 0; s < spinors; ++s) {
    sp.up[s] = up[s];
    sp.dn[s] = dn[s];
    sp.w[s] = weights[s];
  }
  for (int k = 0; k < 4; ++k) sp.n[k] = density[k];
  sp.count = spinors;
  XArgs one = a;
  one.batch.count = 0;
  with_engine<T, +1, true>(a.n, [&](auto eng, int threads, int lines, std::size_t lds) {
    using E = decltype(eng);
    if constexpr (SpinorFits<E>::value) {
      const std::size_t ldsTotal = spinor_lds_bytes(lds, a.n);
      if (ldsTotal > kSpinorLdsLimit) throw InternalError();
      // one spinor reads and writes the arrays once: streaming; the spinors of
      // a batch revisit the tile: default-policy accesses
      auto k = spinors > 1 ? x_spinor_density_kernel<E, T, false> : x_spinor_density_kernel<E, T, true>;
      prepare_kernel(k, ldsTotal);
      hipLaunchKernelGGL(k, dim3(ceil_div(a.Y, lines), a.L - a.zBegin, 1), dim3(threads), ldsTotal, stream, eng,
                         one, sp, static_cast<int>(spinor_region_bytes(lds) / sizeof(cx<T>)), tw);
      gpu_check_launch("x_spinor_density", stream);
    } else {
      throw InternalError();
    }
  });
}

template <typename T>
void launch_space_spinor_mix(cx<T>* up, cx<T>* dn, const T* const* potential, long long count,
                             hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  hipLaunchKernelGGL((space_spinor_mix_kernel<T>), dim3(blocks), dim3(256), 0, stream, up, dn, potential[0],
                     potential[1], potential[2], potential[3], count);
  gpu_check_launch("space_spinor_mix", stream);
}

template <typename T>
void launch_space_spin_density(const cx<T>* up, const cx<T>* dn, T* const* density, T weight, long long count,
                               hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  hipLaunchKernelGGL((space_spin_density_kernel<T>), dim3(blocks), dim3(256), 0, stream, up, dn, density[0],
                     density[1], density[2], density[3], weight, count);
  gpu_check_launch("space_spin_density", stream);
}

// acc[i] += in[i] over `count` sparse values (composed value fan, identity L)
template <typename T>
void launch_values_add(cx<T>* acc, const cx<T>* in, long long count, hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  hipLaunchKernelGGL((values_add_kernel<T>), dim3(blocks), dim3(256), 0, stream, acc, in, count);
  gpu_check_launch("values_add", stream);
}

// acc[i] += in[i] * kernel[i] over `count` sparse values (composed fan-in path)
template <typename T>
void launch_values_scale_add(cx<T>* acc, const cx<T>* in, const T* kernel, bool complexKernel, long long count,
                             hipStream_t stream) {
  if (count <= 0) return;
  const unsigned blocks = static_cast<unsigned>(std::min<long long>((count + 255) / 256, 256 * 64));
  if (complexKernel)
    hipLaunchKernelGGL((values_scale_add_kernel<T, true>), dim3(blocks), dim3(256), 0, stream, acc, in, kernel,
                       count);
  else
    hipLaunchKernelGGL((values_scale_add_kernel<T, false>), dim3(blocks), dim3(256), 0, stream, acc, in, kernel,
                       count);
  gpu_check_launch("values_scale_add", stream);
}

}  // namespace dev
}  // namespace spfft
