// Force-included (g++ -include) when tests/golden/make_goldens_mono.py compiles the reference's viso_mono.cpp, and
// that file only.  The fork this project tracks renamed the members of Matrix and VisualOdometry (_val, _n,
// _matcher, _p_matched, _inliers), but viso_mono.cpp still uses the original names, so it does not compile as
// shipped.  The headers are included first under their own names; the aliases then apply to the statements of
// viso_mono.cpp alone, which are compiled unchanged.
#include "matrix.h"
#include "matcher.h"
#include "viso.h"
#define val _val
#define n _n
#define matcher _matcher
#define p_matched _p_matched
#define inliers _inliers
