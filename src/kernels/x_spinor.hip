// Spinor x stages (the 2x2 local potential applied to both components of a
// spinor, and the spin density matrix, with both components' rows in LDS) and
// the composed spinor paths' passes over two space domains, fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template bool x_spinor_fits<double>(int);
template void launch_x_spinor_apply<double>(const XArgs&, int, cx<double>* const*, cx<double>* const*,
                                            const double* const*, bool, const cx<double>*, hipStream_t);
template void launch_x_spinor_density<double>(const XArgs&, int, const cx<double>* const*,
                                              const cx<double>* const*, const double*, double* const*,
                                              const cx<double>*, hipStream_t);
template void launch_space_spinor_mix<double>(cx<double>*, cx<double>*, const double* const*, long long,
                                              hipStream_t);
template void launch_space_spin_density<double>(const cx<double>*, const cx<double>*, double* const*, double,
                                                long long, hipStream_t);

}  // namespace dev
}  // namespace spfft
