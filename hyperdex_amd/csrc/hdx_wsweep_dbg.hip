// hdx_wsweep_dbg.hip — the wave-staged sweep's A/B forms and debug shapes
// (hdx_wsweep.h), each a named variation of another form, and their rows of
// the stored-object sweep's variant table (hdx_variants.h).  Built into
// libhdxhash_dbg.so only (Makefile SRCS_DBG).
#include "hdx_variants.h"
#include "hdx_wsweep.h"

namespace hdx {

namespace {

// The forms, named by variant id.  Each says what it changes against the form
// it derives from; WsweepForm and WsweepProduct are in hdx_wsweep.h.
// Round 3: from the first form (2 passes, 6 objects, 8.5 KiB windows, four
// waves per workgroup, the record span always compiled in)
struct V231 : WsweepForm { static constexpr uint32_t KCAP = 7; };
struct V232 : WsweepForm { static constexpr int NCH = 3; static constexpr uint32_t WB = 14336, KCAP = 11; };
struct V236 : WsweepForm { static constexpr int LOOP = 2; };
struct V239 : WsweepForm { static constexpr bool GAP = true; };
struct V237 : V239 { static constexpr int SHAPE = 1; };
struct V238 : V239 { static constexpr int SHAPE = 2; };
struct V242 : V239 { static constexpr int LOOP = 2; };
struct V243 : V239 { static constexpr int LOOP = 3; static constexpr bool ASM = true; };
struct V246 : V239 { static constexpr int LOOP = 3; static constexpr bool BF = true; };
struct V244 : V246 { static constexpr bool PU = false; };
struct V245 : V239 { static constexpr int LOOP = 13; };
// back from the product, round by round (RECS by the store layout unless set)
struct V298 : WsweepProductNum2 { static constexpr int LOOP = 13; };
struct V313 : WsweepProductNum2 { static constexpr bool RECS = false; static constexpr int SHAPE = 1; };
struct V314 : V313 { static constexpr int SHAPE = 2; };
struct V315 : V313 { static constexpr int SHAPE = 3; };
struct V271 : WsweepProduct { static constexpr int LOOP = 13, PRIO = 0; };  // round 5 before the wave priorities
struct V272 : V271 { static constexpr uint32_t WB = 9216; };
struct V270 : V271 { static constexpr uint32_t WB = 8704, KCAP = 6; };
struct V273 : V271 { static constexpr int NCH = 3; static constexpr uint32_t WB = 14336, KCAP = 11; };
struct V256 : V270 { static constexpr bool XS = false; };
struct V257 : V256 { static constexpr int WPB = 2; };
struct V258 : V256 { static constexpr uint32_t WB = 7936; };
struct V259 : V256 { static constexpr int WPB = 4; };  // round 4's product
struct V254 : V259 { static constexpr bool DL = true; };
struct V250 : V259 { static constexpr bool RECS = false; };
struct V251 : V250 { static constexpr bool KUNITS = false; };
struct V252 : V250 { static constexpr int SHAPE = 3; };
struct V253 : V250 { static constexpr bool DL = true; };
struct V255 : V250 { static constexpr int SHAPE = 4; };

// These forms need coordinates to write; hipErrorInvalidValue (also: a wider
// schema than the form's passes hold, one NUM2 does not take) leaves the
// sweep to the product (launch_hash_encoded).
template <auto LAUNCH>
hipError_t with_coords(const EncodedArgs& a, hipStream_t stream) {
    return a.coords ? LAUNCH(a, stream) : hipErrorInvalidValue;
}
template <class F>
constexpr auto fixed = with_coords<launch_wsweep_t<F>>;
template <class F>
constexpr auto split = with_coords<by_store_layout<F>>;

const SweepRow kRows[] = {
    {230, with_coords<launch_hash_wsweep_product>, "the product sweep"},
    {231, fixed<V231>, "round 3's form with 7 objects per wave"},
    {232, fixed<V232>, "round 3's form with 3 passes, 11 objects per wave, 14 KiB windows"},
    {236, fixed<V236>, "round 3's product without the pass-boundary gap"},
    {237, fixed<V237>, "debug shape of 239: no hash (WRONG coordinates)"},
    {238, fixed<V238>, "debug shape of 239: no hash, no walk (WRONG coordinates)"},
    {239, fixed<V239>, "round 3's product with the one-block > 64-byte loop (LOOP 1)"},
    {242, fixed<V242>, "round 3's product without the shared final mix16 (LOOP 2)"},
    {243, fixed<V243>, "round 3's product with the DMA as inline asm (4.24 vs 4.20 ms per 10 M: the builtin stays)"},
    {244, fixed<V244>, "246 with the pass loop not unrolled"},
    {245, fixed<V245>, "round 3's product with TNUM, the branchy class and guarded loads"},
    {246, fixed<V246>, "round 3's product without TNUM"},
    {250, fixed<V250>, "259 without the record span"},
    {251, fixed<V251>, "250 with the keys in place gathered by dwords (round 3)"},
    {252, fixed<V252>, "debug shape of 250: no copy, no walk, the hash on made-up descriptors (WRONG coordinates)"},
    {253, fixed<V253>, "250 with round 3's per-KiB span copy"},
    {254, fixed<V254>, "259's record form with round 3's per-KiB span copy"},
    {255, fixed<V255>, "250 with the walk's reads as dword pairs + v_alignbyte (round 3)"},
    {256, split<V256>, "259 with one wave per workgroup"},
    {257, split<V257>, "259 with two waves per workgroup"},
    {258, split<V258>, "256 with 7.75 KiB windows: 17 waves per CU"},
    {259, split<V259>, "round 4's product: four waves per workgroup"},
    {270, split<V270>, "256 with the XCD-aware block order"},
    {271, split<V271>, "270 with 7 objects per wave in 9.5 KiB windows"},
    {272, split<V272>, "270 with 7 objects per wave in 9 KiB windows"},
    {273, split<V273>, "270 with 3 passes, 11 objects per wave, 14 KiB windows"},
    {277, split<V271>, "the product before round 5's wave priorities (= 271)"},
    {293, split<WsweepProductNum2>, "the product with NUM2 whatever the schema (numerics by selects, the class table)"},
    {298, split<V298>, "the product as before LOOP 4 (LOOP 13: two head reads per divergent pass)"},
    {313, fixed<V313>, "debug shape of the product: no hash (WRONG coordinates)"},
    {314, fixed<V314>, "debug shape of the product: no hash, no walk (WRONG coordinates)"},
    {315, fixed<V315>, "debug shape of the product: no copy, no walk (WRONG coordinates)"},
};

}  // namespace

VariantRows<EncodedArgs> wsweep_variant_rows() { return kRows; }

}  // namespace hdx
