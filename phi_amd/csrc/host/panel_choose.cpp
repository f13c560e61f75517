// panel_choose.cpp -- phi_panel_choose of include/phi_host.h: the rule of panel_choose.h behind the C ABI.
#include "panel_choose.h"
#include "../../../include/phi_host.h"

extern "C" int phi_panel_choose(const int32_t *S, int32_t n_blocks, int32_t n_walks, const uint8_t *always, int32_t n_want, uint8_t *keep,
                                int32_t *round_of)
{
    return phi_panel_choose_rule(S, n_blocks, n_walks, always, n_want, keep, round_of, nullptr) ? PHI_HOST_ERR_INVALID : PHI_HOST_OK;
}
