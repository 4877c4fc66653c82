// Force-included (g++ -include) when tests/recon_ref.py compiles the reference's reconstruction.cpp, and that file
// only.  The fork this project tracks renamed Matrix::val to _val, but reconstruction.cpp still says val, so it does
// not compile as shipped.  Every header it uses is included first under its own names; the alias then applies to the
// statements of reconstruction.cpp alone, which are compiled unchanged.
#include <fstream>
#include <iostream>

#include "matrix.h"
#include "matcher.h"
#include "reconstruction.h"
#define val _val
