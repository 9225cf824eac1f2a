// ORACLE support (test infrastructure, CPU only) -- not part of the shipped engine.
// Stand-in header for `make ref`: it lets the reference's own, unmodified translation units compile where the library
// they include is absent.  Rule for every file under oracle/shim/: no arithmetic, no table, nothing taken from VOLK,
// nng or SDR++ -- only the names the reference's sources mention, written here from those uses.
// <dsp/types.h>: dvbs2/s2_defs.h, dvbs2/codings/s2_scrambling.{h,cpp} and common/dsp/demod/constellation.h (through
// dvbs2/codings/modcod_to_cfg.h) use complex_t as a pair of float fields named re and im: they assign them, negate them and
// copy the struct, nothing else.  So the struct below has the two fields and NO operators or methods; a translation unit that
// needs complex arithmetic (common/dsp/demod/constellation.cpp) does not compile over it, on purpose, and stays unpinned.
#pragma once

namespace dsp {
    struct complex_t {
        float re;
        float im;
    };
}
