// pvol_single_exp.hip -- VolumeIntegrator "single" over an exponential medium: pvol_single.hip compiled with
// ExponentialDensity::Density as the density region (pvol_region_exp.h).
#include "pvol_region_exp.h"
#include "pvol_single.hip"
