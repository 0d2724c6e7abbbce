// The row-streaming step's "Y is given" instances (FRONT_STEP_GIVEN: PsglaTvStep.data_term 1), a translation
// unit of their own so that they compile beside the inpainting instances of tv_stream.hip.
#define PSGLA_STREAM_FRONT FRONT_STEP_GIVEN
#include "tv_stream.hip"
