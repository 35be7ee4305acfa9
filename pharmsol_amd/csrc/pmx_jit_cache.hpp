// pmx_jit_cache.hpp — content-addressed cache of hiprtc code objects, in front of jit_compile (pmx_jit.cpp).
//
// Two levels: a process-wide LRU map (always on unless PMX_JIT_CACHE=0) and, when PMX_JIT_CACHE_DIR names a directory,
// one file per key in it.  The key is a 128-bit hash over everything that determines the code object (pmx_jit.cpp
// jit_compile feeds it: cache format, embedded headers, translation unit, options, target, compiler identity); the
// number of bytes hashed travels with every record and is checked again on a hit.  Nothing here can fail a compile:
// every cache error falls through to the compiler.
#pragma once

#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/pmx.h"

namespace pmx {

// bump when the key material or the file layout changes: older files then miss (their names differ) or are rejected
constexpr uint32_t kJitCacheFormat = 1;

// Two independent 64-bit streams over the same bytes (A: FNV-1a; B: rotate-xor-multiply with another odd constant),
// each finished with a 64-bit avalanche that also folds the length in.  Every field is fed with its length in front,
// so ("ab", "c") and ("a", "bc") differ.
struct JitKey {
  uint64_t h[2] = {0, 0};
  uint64_t length = 0;  // bytes of key material hashed
  std::string hex() const;
  bool operator==(const JitKey& o) const { return h[0] == o.h[0] && h[1] == o.h[1] && length == o.length; }
};
class JitKeyHasher {
 public:
  void bytes(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    uint64_t a = a_, b = b_;
    for (size_t i = 0; i < n; ++i) {
      a = (a ^ c[i]) * 0x100000001b3ull;
      b = (((b << 5) | (b >> 59)) ^ c[i]) * 0x9e3779b97f4a7c15ull;
    }
    a_ = a;
    b_ = b;
    n_ += n;
  }
  void u64(uint64_t v) { bytes(&v, sizeof v); }
  void field(const void* p, size_t n) {
    u64(n);
    bytes(p, n);
  }
  void field(const std::string& s) { field(s.data(), s.size()); }
  void field(const char* s) { field(s, std::strlen(s)); }
  JitKey finish() const;

 private:
  uint64_t a_ = 0xcbf29ce484222325ull, b_ = 0x2545f4914f6cdd1dull, n_ = 0;
};
// the same two streams over a code object, folded to 64 bits: the checksum of a cache file's code section
uint64_t jit_checksum(const void* p, size_t n);

// The code object of `key`: from memory, from disk, or from `compile` (called at most once per call, outside every
// lock; its result is stored only if it returns true).  Two threads asking for the same missing key: the second
// waits for the first and takes its result - or compiles itself if the first one failed, so that it gets the log.
// One difference from a compile besides the time: a hit returns an EMPTY *log.  The warnings of a compile that
// succeeded are handed out once, by the call that compiled; they are not stored with the code object.
using JitCompileFn = std::function<bool(std::vector<char>* code, std::string* log)>;
bool jit_cache_get(const JitKey& key, const JitCompileFn& compile, std::vector<char>* code, std::string* log);

}  // namespace pmx
