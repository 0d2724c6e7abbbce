// The row-streaming step's PnP-ULA instances (FRONT_ULA: psgla_tv_ula_step), a translation unit of their own so
// that they compile beside the inpainting and given-Y instances, whose code this front leaves as it was.  The ULA
// step always keeps the TV primal in buffers of its own: no alpha == 1 instances.
#define PSGLA_STREAM_FRONT FRONT_ULA
#define PSGLA_STREAM_NO_ALPHA1
#include "tv_stream.hip"
