// The small-batch tile step's "Y is given" instances (FRONT_STEP_GIVEN: PsglaTvStep.data_term 1), a translation
// unit of their own so that they compile beside the inpainting instances of tv_tile.hip.
#define PSGLA_TILE_FRONT FRONT_STEP_GIVEN
#include "tv_tile.hip"
