// Variant codes: the number a conv launch answers with (ConvPlan::variant, launch_conv's cfg_out, the `cfg` of a profile record and
// of an OU_TRACE line) and the number ConvArgs::force_cfg asks for.  Every range is written ONCE, in kVariantRanges; the launchers
// take their bases from it by name (variant_base), the dispatcher and the walk ask the predicates below, and everything outside
// the library asks ou_variant_family (include/ouniverse_tuning.h; open_universe_amd/variants.py).  Pure host code.
#pragma once
#include <climits>

namespace ou {

struct VariantRange {
  int lo, hi;        // [lo, hi)
  const char* name;  // the finest partition anyone asks for; coarser users group names
};
// Sorted by `lo`; a code belongs to the FIRST range that holds it.  Two overlaps, both historical and both kept as they are
// (DESIGN.md 4.6.3):
//  * block3 inside direct4: launch_conv_block3 (EXPERIMENTS builds) answers 300 + tn = 301 / 302.  conv_direct4_kernel answers
//    300 + 10 TM + log2(WK) with TM >= 1, so no record of its own has these codes -- but as a force_cfg they reach direct4;
//  * recurrence over the tail of split: a force_cfg of 800 .. 1099 reaches conv_split_kernel (which answers 803 .. 925, 85x from
//    conv_splitw_kernel), while every profile RECORD from 1000 on is a GRU pass of (code - 1000) steps (is_recurrence_record).
constexpr VariantRange kVariantRanges[] = {
    {0, 40, "lds"},           // index into kConvCfgs (conv_mfma_kernel)
    {40, 45, "rate_down"},    // 40 + R (rate_down_kernel)
    {45, 50, "rate_up"},      // 45 + R (rate_up_kernel)
    {50, 66, "direct"},       // 50 + 10 tn + GP: 6x / 7x, conv_direct_kernel (first generation, dword loads)
    {66, 68, "direct2"},      // 56 / 57 + 10 tn: 66 / 76 eight K slices, 67 / 77 four (conv_direct2_kernel)
    {68, 76, "direct"},
    {76, 78, "direct2"},
    {78, 80, "direct"},
    {80, 100, "strided"},     // 80 + 10 (tn - 1) + G: conv_direct_strided_kernel
    {100, 200, "fused"},      // fused ConvBlock bodies (launch_chain); as a force_cfg: the first-generation family (105 .. 110)
    {200, 260, "direct3"},    // 200 + 10 TM + KW (conv_direct3_kernel)
    {260, 270, "direct3s"},   // 260 + R (conv_direct3s_kernel)
    {270, 300, "direct3"},
    {300, 400, "direct4"},    // 300 + 10 TM + log2(WK) (conv_direct4_kernel)
    {301, 303, "block3"},     // 300 + tn (conv_block3_kernel) -- overlap, see above
    {400, 500, "direct2w"},   // 400 + 10 WK + KW (conv_direct2w_kernel)
    {500, 600, "direct3w"},   // 500 + 10 TM + KW (conv_direct3w_kernel)
    {600, 800, "direct4w"},   // 600 / 700 (eight / four K slices) + 10 TM + KW (conv_direct4w_kernel)
    {800, 1100, "split"},     // 800 + 100 (TNW == 2) + 10 log2(WM) + KW (conv_split_kernel); 850 + 10 log2(WM) + KW (conv_splitw_kernel)
    {1000, INT_MAX, "recurrence"},  // 1000 + steps of a GRU pass -- overlap, see above
};

constexpr bool variant_name_is(const char* a, const char* b) {
  while (*a && *a == *b) { a++; b++; }
  return *a == *b;
}
// the name of the first range holding `code`, or null
constexpr const char* variant_family(int code) {
  for (const VariantRange& r : kVariantRanges)
    if (code >= r.lo && code < r.hi) return r.name;
  return nullptr;
}
// first code of the first / one past the last code of the last range called `name`
constexpr int variant_base(const char* name) {
  for (const VariantRange& r : kVariantRanges)
    if (variant_name_is(r.name, name)) return r.lo;
  return -1;
}
constexpr int variant_end(const char* name) {
  int hi = -1;
  for (const VariantRange& r : kVariantRanges)
    if (variant_name_is(r.name, name)) hi = r.hi;
  return hi;
}
constexpr bool variant_in(int code, const char* name) {
  const char* f = variant_family(code);
  return f && variant_name_is(f, name);
}

constexpr bool variant_ranges_sorted() {
  const int n = sizeof(kVariantRanges) / sizeof(kVariantRanges[0]);
  for (int i = 0; i + 1 < n; i++) {
    const VariantRange &a = kVariantRanges[i], &b = kVariantRanges[i + 1];
    const bool documented = variant_name_is(b.name, "block3") || variant_name_is(b.name, "recurrence");
    if (a.lo >= a.hi || b.lo < a.lo || (b.lo < a.hi && !documented)) return false;
    if (variant_name_is(a.name, "block3") && b.lo < kVariantRanges[i - 1].hi) return false;  // (the range behind the inner one)
  }
  return true;
}
static_assert(variant_ranges_sorted(), "kVariantRanges: sorted by lo, disjoint but for the two documented overlaps");

// the bases the launchers add their shape digits to
constexpr int kVarRateDown = variant_base("rate_down"), kVarRateUp = variant_base("rate_up");
constexpr int kVarDirect = variant_base("direct"), kVarStrided = variant_base("strided");
constexpr int kVarDirect2 = kVarDirect + 6;  // + 10 tn (+ 1: four K slices): 66 / 76 / 67 / 77
constexpr int kVarFused = variant_base("fused");
constexpr int kVarDirect3 = variant_base("direct3"), kVarDirect3s = variant_base("direct3s");
constexpr int kVarDirect4 = variant_base("direct4");  // (launch_conv_block3 writes its 300 + tn itself: experiments only)
constexpr int kVarDirect2w = variant_base("direct2w"), kVarDirect3w = variant_base("direct3w");
constexpr int kVarDirect4w = variant_base("direct4w"), kVarDirect4w4 = kVarDirect4w + 100;  // eight / four K slices
constexpr int kVarSplit = variant_base("split"), kVarSplitw = kVarSplit + 50;
constexpr int kVarRecurrence = variant_base("recurrence");
static_assert(variant_in(kVarDirect2 + 10, "direct2") && variant_in(kVarDirect2 + 21, "direct2") && !variant_in(kVarDirect2 + 12, "direct2") &&
                  variant_in(kVarDirect4w4, "direct4w") && variant_in(kVarSplitw, "split"),
              "derived bases lie in their ranges");

// the wide-load split-K kernels (conv_direct2_kernel, conv_direct2w_kernel): what launch_conv_direct's block -> tile maps ask
inline bool is_direct2(int code) { return variant_in(code, "direct2") || variant_in(code, "direct2w"); }
inline bool is_fused_body(int code) { return variant_in(code, "fused"); }
// a profile record (not a force_cfg) of a GRU pass
inline bool is_recurrence_record(int code) { return code >= kVarRecurrence; }
// Does the kernel behind a variant code honour ConvArgs::lens in its epilogue?  Every conv family but the fused ConvBlock bodies (their conv1 / conv2 tiles live in LDS, where nothing zeroes them behind a
// row's end -- the runner does not fuse ragged batches) keeps ConvArgs::lens in its epilogue.
inline bool conv_masks_rows(int code) { return code >= 0 && !is_fused_body(code); }

}  // namespace ou
