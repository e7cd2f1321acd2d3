// Exchange pair operator x stages (forward: rows conj(a) * b; backward: acc += w a u
// from LDS) and the composed path's two one-pass space-domain kernels, fp64 transforms.
#include "kernels/stage_launch.hpp"

namespace spfft {
namespace dev {

template void launch_x_forward_pair<double>(const XArgs&, const cx<double>*, const cx<double>*, cx<double>*,
                                            const cx<double>*, hipStream_t);
template void launch_x_backward_fock<double>(const XArgs&, const cx<double>*, const cx<double>*, cx<double>*,
                                             double, const cx<double>*, hipStream_t);
template void launch_space_pair<double>(void*, const double*, const double*, long long, bool, hipStream_t);
template void launch_space_fock<double>(const void*, const double*, double*, double, long long, bool,
                                        hipStream_t);

}  // namespace dev
}  // namespace spfft
