// rfx_czt_list.hip - translation unit 1 of the chirp-z engine: the Griffin-Lim kernels that walk the free-frame list of a held call
// (include/rfx.h: rfx_held_call_options; rfx_guide_core.h) and their launcher.  See the head of rfx_czt.hip.
#define RFX_CZT_LIST_TU 1
#include "rfx_czt.hip"
