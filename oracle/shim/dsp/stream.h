// ORACLE support (test infrastructure, CPU only) -- not part of the shipped engine.
// Stand-in header for `make ref`: it lets the reference's own, unmodified translation units compile where the library
// they include is absent.  Rule for every file under oracle/shim/: no arithmetic, no table, nothing taken from VOLK,
// nng or SDR++ -- only the names the reference's sources mention, written here from those uses.
// <dsp/stream.h>: dvbs2/bbframe_ts_parser.h includes it and uses nothing from it.  Empty on purpose.
#pragma once
