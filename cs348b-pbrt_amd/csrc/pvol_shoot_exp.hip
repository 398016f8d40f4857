// pvol_shoot_exp.hip -- the photon shooter through an exponential medium: pvol_shoot.hip compiled with ExponentialDensity::Density
// as the density region (pvol_region_exp.h).
#include "pvol_region_exp.h"
#include "pvol_shoot.hip"
