// ORACLE support (test infrastructure, CPU only) -- not part of the shipped engine.
// Stand-in header for `make ref`: it lets the reference's own, unmodified translation units compile where the library
// they include is absent.  Rule for every file under oracle/shim/: no arithmetic, no table, nothing taken from VOLK,
// nng or SDR++ -- only the names the reference's sources mention, written here from those uses.
// <volk/volk_alloc.hh>: cc_common.h and cc_decoder.h use volk::vector<T> as a container (resize, data); the aligned allocator
// of the real one changes no value.  cc_decoder.h / cc_decoder.cpp also rely on the standard headers below arriving through
// this one (uint8_t, std::string, std::ostringstream, std::runtime_error).
#pragma once
#include <cstdint>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace volk {
template <class T>
using vector = std::vector<T>;
}
