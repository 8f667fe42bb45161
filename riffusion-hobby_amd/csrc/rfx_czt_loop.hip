// rfx_czt_loop.hip - translation unit 2 of the chirp-z engine: the forward kernels of a loop call (include/rfx.h: rfx_stft_loop and the
// other *_loop forward entries; rfx_czt_stft_kernel.hip.h with the row read modulo its length) and their launcher.  See the head of
// rfx_czt.hip.
#define RFX_CZT_LOOP_TU 1
#include "rfx_czt.hip"
