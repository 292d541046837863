// Host harness around vbz_compression_amd/csrc/xxh64.h (tests only): the serial XXH64 the device kernel is held to, built with g++.
#include "xxh64.h"

extern "C" uint64_t h_xxh64(const uint8_t* p, uint64_t len) { return vbzhip::xxh64(p, len); }
