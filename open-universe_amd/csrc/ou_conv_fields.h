// Fields of ConvArgs that a plan_* function derives from the layer shape, each written once.  Pure host code.
#pragma once
#include "ou_kernels.h"

namespace ou {

// exact for the index ranges used (e < 2^13, divisor < 2^11): floor(e/d) == umulhi(e, 2^32/d + 1)
inline unsigned magic_div(unsigned d) { return (unsigned)(0x100000000ull / d) + 1u; }
inline void fill_magic_up(ConvArgs& aa) { aa.magic_up = aa.up == 1 ? 0u : magic_div((unsigned)aa.up); }
inline void fill_magic_span(ConvArgs& aa) {
  const int bns[3] = {128, 64, 32};
  for (int i = 0; i < 3; i++) aa.magic_span[i] = magic_div((unsigned)((bns[i] - 1) * aa.stride + aa.KW));
}

// Which operand an XCD's L2 owns: memory-side bytes ~ 8 X + W (slabs, map 1) vs X + 8 W (time tiles, map 2); needs aa.grid_m /
// aa.grid_n.  `map2d`: the direct family's 2-D extension for its wide-load kernels -- called where the rule arrives at map 2 and
// the row tiles pair up; it answers the map to use instead (3) or 2.  `tuned`: that family's own override (ConvArgs::d2_map),
// applied before force_xcd_map; `allow_2d`: whether maps 3 / 4 exist for the kernel at all.
template <class Map2d>
inline void fill_xcd_map(ConvArgs& aa, bool allow_2d, int tuned, Map2d map2d) {
  const double xb = (double)aa.Cin * aa.Nq * aa.stride, wb = (double)aa.M * aa.Cin * aa.KW;
  aa.xcd_map = 0;
  if (aa.grid_m % 8 == 0 && wb >= xb) aa.xcd_map = 1;
  else if (aa.grid_n >= 8) aa.xcd_map = 2;
  if (allow_2d && aa.xcd_map == 2 && aa.grid_m % 2 == 0) aa.xcd_map = map2d();
  if (allow_2d && tuned >= 0) aa.xcd_map = tuned;
  if (aa.force_xcd_map >= 0) aa.xcd_map = aa.force_xcd_map;
  if (aa.xcd_map == 1 && aa.grid_m % 8) aa.xcd_map = 0;
  if ((aa.xcd_map == 3 || aa.xcd_map == 4) && !allow_2d) aa.xcd_map = 0;
}
inline void fill_xcd_map(ConvArgs& aa) { fill_xcd_map(aa, false, -1, [] { return 2; }); }

}  // namespace ou
