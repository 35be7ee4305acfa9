// pmx_jit_cache.cpp — the two levels of the code-object cache (pmx_jit_cache.hpp) and its C entry points.
#include "pmx_jit_cache.hpp"

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdio>
#include <list>
#include <mutex>
#include <set>
#include <unordered_map>

#include "pmx_internal.hpp"

namespace pmx {

namespace {

uint64_t avalanche(uint64_t x) {  // (the 64-bit finalizer of MurmurHash3)
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

constexpr char kFileSuffix[] = ".pmxjit";
constexpr size_t kHexLen = 32;

// ---- disk level: [magic u64][format u32][0 u32][key u64 x2][key-material length u64][code size u64][checksum u64][code]
constexpr uint64_t kMagic = 0x0154494a584d50ull;  // "PMXJIT\1\0" read as a little-endian u64
constexpr size_t kHeaderBytes = 56;
constexpr size_t kMaxFileBytes = size_t{1} << 30;  // far above any code object (the largest so far: 1.5 MB); a larger file is refused unread

void put64(unsigned char* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = static_cast<unsigned char>(v >> (8 * i));
}
uint64_t get64(const unsigned char* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  return v;
}

void make_dirs(const std::string& dir) {  // mkdir -p; a failure shows up as a failed open later
  for (size_t i = 1; i <= dir.size(); ++i)
    if (i == dir.size() || dir[i] == '/') (void)::mkdir(dir.substr(0, i).c_str(), 0777);
}

std::string file_of(const std::string& dir, const JitKey& key) { return dir + "/" + key.hex() + kFileSuffix; }

enum DiskRead { DISK_MISS, DISK_REJECT, DISK_HIT };
DiskRead disk_read(const std::string& dir, const JitKey& key, std::vector<char>* code) {
  const int fd = ::open(file_of(dir, key).c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) return (errno == ENOENT || errno == ENOTDIR) ? DISK_MISS : DISK_REJECT;
  struct stat st;
  std::vector<unsigned char> buf;
  bool ok = ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && static_cast<size_t>(st.st_size) > kHeaderBytes &&
            static_cast<size_t>(st.st_size) <= kMaxFileBytes;
  if (ok) {
    buf.resize(static_cast<size_t>(st.st_size));
    size_t got = 0;
    while (got < buf.size()) {
      const ssize_t n = ::read(fd, buf.data() + got, buf.size() - got);
      if (n < 0 && errno == EINTR) continue;
      if (n <= 0) break;
      got += static_cast<size_t>(n);
    }
    ok = got == buf.size();
  }
  ::close(fd);
  if (!ok) return DISK_REJECT;
  const unsigned char* h = buf.data();
  const size_t ncode = buf.size() - kHeaderBytes;
  if (get64(h) != kMagic || get64(h + 8) != kJitCacheFormat || get64(h + 16) != key.h[0] || get64(h + 24) != key.h[1] ||
      get64(h + 32) != key.length || get64(h + 40) != ncode || get64(h + 48) != jit_checksum(h + kHeaderBytes, ncode))
    return DISK_REJECT;
  code->assign(reinterpret_cast<const char*>(h) + kHeaderBytes, reinterpret_cast<const char*>(h) + buf.size());
  return DISK_HIT;
}

// Written under a name of its own in the same directory, then renamed: a reader sees the whole file or none, and
// processes that write the same key at the same time replace each other's (identical) file.
bool disk_write(const std::string& dir, const JitKey& key, const std::vector<char>& code) {
  static std::atomic<uint64_t> serial{0};
  make_dirs(dir);
  const std::string path = file_of(dir, key);
  const std::string tmp = path + ".tmp." + std::to_string(static_cast<long long>(::getpid())) + "." + std::to_string(serial++);
  const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0600);  // (for the owner alone: the file is loaded as GPU code)
  if (fd < 0) return false;
  unsigned char h[kHeaderBytes];
  put64(h, kMagic);
  put64(h + 8, kJitCacheFormat);
  put64(h + 16, key.h[0]);
  put64(h + 24, key.h[1]);
  put64(h + 32, key.length);
  put64(h + 40, code.size());
  put64(h + 48, jit_checksum(code.data(), code.size()));
  auto write_all = [fd](const void* p, size_t n) {
    const char* c = static_cast<const char*>(p);
    while (n > 0) {
      const ssize_t w = ::write(fd, c, n);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) return false;
      c += w;
      n -= static_cast<size_t>(w);
    }
    return true;
  };
  bool ok = write_all(h, sizeof h) && write_all(code.data(), code.size());
  ok = (::close(fd) == 0) && ok;
  ok = ok && ::rename(tmp.c_str(), path.c_str()) == 0;
  if (!ok) (void)::unlink(tmp.c_str());
  return ok;
}

// the cache's own files in `dir` (32 hex digits + suffix, and temporaries of those): nothing else is ever removed
void disk_clear(const std::string& dir) {
  DIR* d = ::opendir(dir.c_str());
  if (!d) return;
  std::vector<std::string> names;
  while (const dirent* e = ::readdir(d)) {
    const std::string n = e->d_name;
    if (n.size() < kHexLen + sizeof kFileSuffix - 1 || n.compare(kHexLen, sizeof kFileSuffix - 1, kFileSuffix) != 0) continue;
    if (n.find_first_not_of("0123456789abcdef") != kHexLen) continue;
    names.push_back(n);
  }
  ::closedir(d);
  for (const auto& n : names) (void)::unlink((dir + "/" + n).c_str());
}

// ---- memory level
struct Entry {
  JitKey key;
  std::vector<char> code;
};
struct Cache {
  std::mutex mu;
  std::condition_variable cv;
  std::list<Entry> lru;  // front = most recently used
  std::unordered_map<std::string, std::list<Entry>::iterator> by_hex;
  std::set<std::string> in_flight;  // keys some thread is loading or compiling right now
  int64_t bytes = 0;
  pmx_jit_cache_counters n{};
  void drop(std::list<Entry>::iterator it) {
    bytes -= static_cast<int64_t>(it->code.size());
    by_hex.erase(it->key.hex());
    lru.erase(it);
  }
  void trim(size_t max_entries) {
    while (lru.size() > max_entries) drop(std::prev(lru.end()));
  }
};
Cache& cache() {
  static Cache* c = new Cache;  // (never destroyed: models may be created from other static destructors)
  return *c;
}

}  // namespace

std::string JitKey::hex() const {
  char buf[kHexLen + 1];
  std::snprintf(buf, sizeof buf, "%016llx%016llx", static_cast<unsigned long long>(h[0]), static_cast<unsigned long long>(h[1]));
  return buf;
}

JitKey JitKeyHasher::finish() const {
  JitKey k;
  k.h[0] = avalanche(a_ ^ n_);
  k.h[1] = avalanche(b_ + 0x9e3779b97f4a7c15ull * n_);
  k.length = n_;
  return k;
}

uint64_t jit_checksum(const void* p, size_t n) {
  JitKeyHasher h;
  h.bytes(p, n);
  const JitKey k = h.finish();
  return k.h[0] ^ ((k.h[1] << 1) | (k.h[1] >> 63));
}

bool jit_cache_get(const JitKey& key, const JitCompileFn& compile, std::vector<char>* code, std::string* log) {
  const Tunables tun = tunables();
  Cache& c = cache();
  if (!tun.jit_cache) {
    {
      std::lock_guard<std::mutex> lock(c.mu);
      ++c.n.compiles;
    }
    return compile(code, log);
  }
  const std::string hex = key.hex();
  {
    std::unique_lock<std::mutex> lock(c.mu);
    for (;;) {
      auto it = c.by_hex.find(hex);
      if (it != c.by_hex.end() && it->second->key == key) {
        c.lru.splice(c.lru.begin(), c.lru, it->second);
        *code = it->second->code;
        log->clear();
        ++c.n.mem_hits;
        return true;
      }
      if (c.in_flight.count(hex) == 0) break;
      c.cv.wait(lock);
    }
    c.in_flight.insert(hex);
  }
  // from here on the key is ours: whatever happens below - an exception included - it is handed back and waiters are woken
  struct InFlight {
    Cache& c;
    const std::string& hex;
    ~InFlight() {
      {
        std::lock_guard<std::mutex> lock(c.mu);
        c.in_flight.erase(hex);
      }
      c.cv.notify_all();
    }
  } in_flight{c, hex};
  const std::string dir = tun.jit_cache_dir ? tun.jit_cache_dir : "";
  DiskRead dr = DISK_MISS;
  bool ok = false, compiled = false, written = false;
  try {
    if (!dir.empty()) dr = disk_read(dir, key, code);
  } catch (const std::exception&) {  // (out of memory on a file of the right name: refused like any other bad file)
    dr = DISK_REJECT;
  }
  if (dr == DISK_HIT) {
    ok = true;
    log->clear();
  } else {
    compiled = true;
    try {
      ok = compile(code, log);
    } catch (const std::exception& e) {  // nothing thrown may leave through the C entry points
      *log = std::string("compiling the model: ") + e.what();
      ok = false;
    }
    try {
      if (ok && !dir.empty()) written = disk_write(dir, key, *code);
    } catch (const std::exception&) {
      written = false;
    }
  }
  std::lock_guard<std::mutex> lock(c.mu);
  c.n.compiles += compiled;
  c.n.disk_hits += dr == DISK_HIT;
  c.n.disk_rejects += dr == DISK_REJECT;
  c.n.disk_writes += written;
  if (ok) {
    try {
      auto it = c.by_hex.find(hex);
      if (it != c.by_hex.end()) c.drop(it->second);  // (same hash, other length: the newer one stays)
      c.lru.push_front(Entry{key, *code});
      c.by_hex[hex] = c.lru.begin();
      c.bytes += static_cast<int64_t>(code->size());
      c.trim(static_cast<size_t>(tun.jit_cache_entries));
    } catch (const std::exception&) {  // no room to remember it: start the memory level afresh, the caller has its code object
      c.lru.clear();
      c.by_hex.clear();
      c.bytes = 0;
    }
  }
  return ok;
}

}  // namespace pmx

extern "C" {

int32_t pmx_jit_cache_stats(pmx_jit_cache_counters* out) {
  if (!out) return fail(PMX_ERR_INVALID_ARGUMENT, "out is null");
  pmx::Cache& c = pmx::cache();
  std::lock_guard<std::mutex> lock(c.mu);
  *out = c.n;
  out->entries = static_cast<int64_t>(c.lru.size());
  out->bytes = c.bytes;
  return PMX_OK;
}

void pmx_jit_cache_clear(int32_t also_disk) {
  pmx::Cache& c = pmx::cache();
  {
    std::lock_guard<std::mutex> lock(c.mu);
    c.lru.clear();
    c.by_hex.clear();
    c.bytes = 0;
    c.n = pmx_jit_cache_counters{};
  }
  if (also_disk) {
    const pmx::Tunables tun = pmx::tunables();
    if (tun.jit_cache_dir && tun.jit_cache_dir[0]) pmx::disk_clear(tun.jit_cache_dir);
  }
}

}  // extern "C"
