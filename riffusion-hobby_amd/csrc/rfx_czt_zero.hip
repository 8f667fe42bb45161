// rfx_czt_zero.hip - translation unit 3 of the chirp-z engine: the forward kernels of the zero-extended analysis (include/rfx.h:
// rfx_istft_backward; rfx_czt_stft_kernel.hip.h with the row read under zero_outside) and their launcher.  See the head of rfx_czt.hip.
#define RFX_CZT_LOOP_TU 2
#include "rfx_czt.hip"
