// tfg_fused_prec_sat.hip -- the fp32 engine's Satterlund form with the fp64
// fluxes (SATTERLUND: true and tfg_set_flux(h, TFG_FLUX_F64)): the
// instantiations k_fused<float, false, ..., PREC = true, SAT = true>
// (tfg_fused.hpp, tfg::cell_step_fast) and their launch.  Its own translation
// unit so that the library's units still compile side by side (build()).
#include "tfg_fused.hpp"

namespace tfg_kern {

template hipError_t launch_fused_fast<true, true>(const KArgs&, const FusedBufs&, bool, bool, bool, bool, int, size_t,
                                                  hipStream_t);

}  // namespace tfg_kern
