// The row-streaming PnP-ULA step's "data gradient is given" instances (FRONT_ULA_GIVEN: psgla_tv_ula_step with
// tv.data_term 2, deblurring), a translation unit of their own so that they compile beside the other fronts'
// instances, whose code this front leaves as it was.  As FRONT_ULA: the x2-separate layout only.
#define PSGLA_STREAM_FRONT FRONT_ULA_GIVEN
#define PSGLA_STREAM_NO_ALPHA1
#include "tv_stream.hip"
