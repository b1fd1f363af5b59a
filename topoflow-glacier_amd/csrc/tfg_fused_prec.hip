// tfg_fused_prec.hip -- the fp32 engine's fp64-flux form (tfg_set_flux(h,
// TFG_FLUX_F64)): the instantiations k_fused<float, false, ..., PREC = true>
// (tfg_fused.hpp, tfg::cell_step_fast) and their launch.  Its own translation
// unit so that the library's units still compile side by side (build()).
#include "tfg_fused.hpp"

namespace tfg_kern {

template hipError_t launch_fused_fast<true, false>(const KArgs&, const FusedBufs&, bool, bool, bool, bool, int, size_t,
                                                   hipStream_t);

}  // namespace tfg_kern
