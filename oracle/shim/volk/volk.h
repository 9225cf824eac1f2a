// ORACLE support (test infrastructure, CPU only) -- not part of the shipped engine.
// Stand-in header for `make ref`: it lets the reference's own, unmodified translation units compile where the library
// they include is absent.  Rule for every file under oracle/shim/: no arithmetic, no table, nothing taken from VOLK,
// nng or SDR++ -- only the names the reference's sources mention, written here from those uses.
// <volk/volk.h>: CCDecoder's constructor (cc_decoder.cpp:58-92) asks the library which implementations of the K=7 r=1/2
// kernel exist and takes "spiral" / "neonspiral" if one is listed.  None is listed here, so the decoder keeps the reference's
// own in-tree volk_fixed::volk_8u_x4_conv_k7_r2_8u_generic (volk_k7_r2_generic_fixed.h:136-163), the kernel the oracle
// restates.  The `manual` dispatcher is named by two wrappers in that header that are then never called: it aborts.
#pragma once
#include <cstddef>
#include <cstdlib>

struct volk_func_desc {
    const char** impl_names;
    size_t n_impls;
};

inline volk_func_desc volk_8u_x4_conv_k7_r2_8u_get_func_desc() { return volk_func_desc{nullptr, 0}; }

inline void volk_8u_x4_conv_k7_r2_8u_manual(unsigned char*, unsigned char*, unsigned char*, unsigned char*, unsigned int,
                                            unsigned int, unsigned char*, const char*) {
    abort();
}
