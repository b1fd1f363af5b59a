// tfg_fused_sat.hip -- the fp32 engine's Satterlund form (SATTERLUND: true in
// the configuration, DevParams::satterlund): the instantiations k_fused<float,
// false, ..., PREC = false, SAT = true> (tfg_fused.hpp, tfg::cell_step_fast)
// and their launch.  Its own translation unit so that the library's units
// still compile side by side (build()).
#include "tfg_fused.hpp"

namespace tfg_kern {

template hipError_t launch_fused_fast<false, true>(const KArgs&, const FusedBufs&, bool, bool, bool, bool, int, size_t,
                                                   hipStream_t);

}  // namespace tfg_kern
