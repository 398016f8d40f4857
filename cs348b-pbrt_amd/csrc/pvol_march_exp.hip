// pvol_march_exp.hip -- Li(), the tile pre-pass and the surface term over an exponential medium: pvol_march.hip compiled with
// ExponentialDensity::Density as the density region (pvol_region_exp.h).
#include "pvol_region_exp.h"
#include "pvol_march.hip"
