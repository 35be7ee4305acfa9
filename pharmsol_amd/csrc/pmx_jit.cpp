#ifndef _GNU_SOURCE
#define _GNU_SOURCE 1
#endif
// pmx_jit.cpp — run-time compilation of user models (hiprtc -> gfx950 code object -> hipModule).  The text that is
// compiled is pmx_jit_source.cpp's.
#include "pmx_jit.hpp"
#include "pmx_devtypes.hpp"
#include "pmx_jit_cache.hpp"

#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "pmx_jit_headers.inc"

namespace pmx {

// The hiprtc entry points: the copy the process linked (inside a PyTorch process: PyTorch's), or - PMX_HIPRTC_LIB=/path/to/
// libhiprtc.so - another one loaded beside it (e.g. the image's newer /opt/rocm/lib/libhiprtc.so, whose compiler builds the
// faster closure kernels: INTEGRATION.md section 6).  Only the compile is taken from it; the code object is loaded by the
// process's own HIP runtime either way.
struct HiprtcApi {
  decltype(&hiprtcCreateProgram) create = &hiprtcCreateProgram;
  decltype(&hiprtcCompileProgram) compile = &hiprtcCompileProgram;
  decltype(&hiprtcGetProgramLogSize) log_size = &hiprtcGetProgramLogSize;
  decltype(&hiprtcGetProgramLog) log = &hiprtcGetProgramLog;
  decltype(&hiprtcGetCodeSize) code_size = &hiprtcGetCodeSize;
  decltype(&hiprtcGetCode) code = &hiprtcGetCode;
  decltype(&hiprtcDestroyProgram) destroy = &hiprtcDestroyProgram;
  decltype(&hiprtcGetErrorString) err = &hiprtcGetErrorString;
  decltype(&hiprtcVersion) version = &hiprtcVersion;
  std::string lib_path;  // PMX_HIPRTC_LIB when that copy is the one in use ("": the linked one)
};
const HiprtcApi& hiprtc_api() {
  static const HiprtcApi api = [] {
    HiprtcApi a;
    const char* path = std::getenv("PMX_HIPRTC_LIB");
    if (!path || !*path) return a;
    // (its own link namespace: hiprtc finds its compiler library - comgr - by name at run time, and in the process's
    // namespace that name is already taken by the copy loaded first)
    void* h = dlmopen(LM_ID_NEWLM, path, RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      std::fprintf(stderr, "libpmx_hip: PMX_HIPRTC_LIB=%s could not be loaded (%s): using the linked hiprtc\n", path, dlerror());
      return a;
    }
    HiprtcApi b;
    bool ok = true;
    auto get = [&](auto& fn, const char* name) {
      void* sym = dlsym(h, name);
      if (!sym) ok = false;
      else fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(sym);
    };
    get(b.create, "hiprtcCreateProgram");
    get(b.compile, "hiprtcCompileProgram");
    get(b.log_size, "hiprtcGetProgramLogSize");
    get(b.log, "hiprtcGetProgramLog");
    get(b.code_size, "hiprtcGetCodeSize");
    get(b.code, "hiprtcGetCode");
    get(b.destroy, "hiprtcDestroyProgram");
    get(b.err, "hiprtcGetErrorString");
    get(b.version, "hiprtcVersion");
    b.lib_path = path;
    return ok ? b : a;
  }();
  return api;
}

namespace {

// one hiprtc compile of `tu`: the code object, or the compiler's diagnostics in *log
bool hiprtc_compile(const HiprtcApi& rt, const std::string& tu, const std::vector<const char*>& opts, std::vector<char>* code,
                    std::string* log) {
  hiprtcProgram prog = nullptr;
  hiprtcResult r = rt.create(&prog, tu.c_str(), "pmx_user_model.hip", kJitHeaderCount, kJitHeaderSources,
                                       kJitHeaderNames);
  if (r != HIPRTC_SUCCESS) {
    *log = std::string("hiprtcCreateProgram: ") + rt.err(r);
    return false;
  }
  r = rt.compile(prog, static_cast<int>(opts.size()), opts.data());
  size_t ls = 0;
  rt.log_size(prog, &ls);
  if (ls > 1) {
    log->assign(ls, '\0');
    rt.log(prog, &(*log)[0]);
  } else {
    log->clear();
  }
  if (r != HIPRTC_SUCCESS) {
    if (log->empty()) *log = rt.err(r);
    rt.destroy(&prog);
    return false;
  }
  size_t cs = 0;
  rt.code_size(prog, &cs);
  code->assign(cs, 0);
  rt.code(prog, code->data());
  rt.destroy(&prog);
  return cs > 0;
}

// What, besides the translation unit and the options, decides the code object and never changes within a process: the
// cache format, the embedded headers, the compiler (hiprtcVersion of the copy that is called + PMX_HIPRTC_LIB's path).
const JitKeyHasher& key_prefix() {
  static const JitKeyHasher prefix = [] {
    const HiprtcApi& rt = hiprtc_api();
    JitKeyHasher h;
    h.u64(kJitCacheFormat);
    h.u64(static_cast<uint64_t>(kJitHeaderCount));
    for (int i = 0; i < kJitHeaderCount; ++i) {
      h.field(kJitHeaderNames[i]);
      h.field(kJitHeaderSources[i]);
    }
    int major = -1, minor = -1;
    if (rt.version(&major, &minor) != HIPRTC_SUCCESS) major = minor = -1;
    h.u64(static_cast<uint64_t>(static_cast<int64_t>(major)));
    h.u64(static_cast<uint64_t>(static_cast<int64_t>(minor)));
    h.field(rt.lib_path);
    // hiprtcVersion is coarse (ROCm 7.0's and 7.2's copies both answer 9.0): the file the compile entry point comes
    // from, its size and its modification time tell two installed copies - and an upgrade in place - apart
    Dl_info info;
    struct stat st;
    if (dladdr(reinterpret_cast<void*>(rt.compile), &info) && info.dli_fname) {
      h.field(info.dli_fname);
      if (::stat(info.dli_fname, &st) == 0) {
        h.u64(static_cast<uint64_t>(st.st_size));
        h.u64(static_cast<uint64_t>(st.st_mtime));
      }
    }
    return h;
  }();
  return prefix;
}

}  // namespace

bool jit_compile(const JitSpec& spec, std::vector<char>* code, std::string* log) {
  const HiprtcApi& rt = hiprtc_api();
  const std::string tu = jit_translation_unit(spec);
  static const std::string kArch = "gfx950", kArchOpt = "--offload-arch=" + kArch;
  std::vector<const char*> opts = {kArchOpt.c_str(), "-O3", "-std=c++17", "-ffp-contract=fast"};
  std::vector<std::string> extra;  // PMX_DEBUG_JIT_OPTS="opt;opt;..." (experiments)
  if (const char* ex = std::getenv("PMX_DEBUG_JIT_OPTS")) {
    std::string cur;
    for (const char* c = ex;; ++c) {
      if (*c == ';' || *c == 0) {
        if (!cur.empty()) extra.push_back(cur);
        cur.clear();
        if (*c == 0) break;
      } else {
        cur.push_back(*c);
      }
    }
    for (auto& e : extra) opts.push_back(e.c_str());
  }
  JitKeyHasher h = key_prefix();
  h.field(kArch);
  h.u64(opts.size());
  for (const char* o : opts) h.field(o);
  h.field(tu);
  const bool ok = jit_cache_get(
      h.finish(), [&](std::vector<char>* c, std::string* l) { return hiprtc_compile(rt, tu, opts, c, l); }, code, log);
  if (!ok) return false;
  if (const char* dump = std::getenv("PMX_DEBUG_JIT_DUMP")) {  // (the code object, for llvm-objdump / llvm-readelf)
    if (FILE* f = std::fopen(dump, "wb")) {
      std::fwrite(code->data(), 1, code->size(), f);
      std::fclose(f);
    }
  }
  return true;
}

hipError_t jit_load(const std::vector<char>& code, JitModule* out, const JitSpec& spec) {
  const JitEntryRow& row = kJitEntries[spec.kind];
  const SolvRange sv = jit_entry_solvers(spec);
  hipError_t e = hipModuleLoadData(&out->module, code.data());
  if (e != hipSuccess) return e;
  for (int mode = 0; mode < 2; ++mode)
    for (int lag = 0; lag < (row.lag ? 2 : 1); ++lag)
      for (int ll = 0; ll < 2; ++ll)
        for (int solv = sv.begin; solv < sv.end; ++solv) {
          e = hipModuleGetFunction(&out->fn[mode][lag][ll][solv], out->module, jit_entry_name(row, mode, lag, ll, solv).c_str());
          if (e != hipSuccess) return e;
        }
  return hipSuccess;
}

void jit_unload(JitModule* m) {
  if (m->module) (void)hipModuleUnload(m->module);
  m->module = nullptr;
}

}  // namespace pmx
