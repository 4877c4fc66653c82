// Force-included (-include) in front of the reference's stereomapper/planeestimation.cpp when
// tests/plane_ref.py builds the reference harness; never part of the library.  The system headers come first, so that
// the three words below are replaced in the reference's own text only:
//   time(x)  -> the seed the harness chose (the reference seeds with srand(time(NULL))),
//   rand     -> a harness function that calls rand() and counts the draws,
//   private  -> public, so that the harness can step sparseDisparityGrid / drawRandomPlaneSample itself.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <iostream>
#include <vector>

time_t plane_harness_time();
int plane_harness_rand();

#define time(x) plane_harness_time()
#define rand plane_harness_rand
#define private public
