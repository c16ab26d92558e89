// jit_cache.hpp — from a generated source to a code object (jit_cache.cpp): hiprtc resolved at run time, and the kernel cache in front of
// it — memory (bounded, LRU) over disk (persistent) over the compiler.  Everything that takes the cache's process-wide lock is here.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace srack {

struct JitKernel;  // a loaded module (jit.hpp)

struct JitCacheStats {  // process-wide, since start (srack_kernel_cache_stats)
    uint64_t compiled = 0, disk_hits = 0, memory_hits = 0, modules_loaded = 0, code_evictions = 0, module_evictions = 0;
    uint64_t resident_code_objects = 0, resident_modules = 0;
    double compile_ms = 0.0;
    char directory[512] = {0};  // the disk cache in use ("" = none)
};

struct CodeObject {
    std::vector<char> code;
};
using CodePtr = std::shared_ptr<const CodeObject>;

struct Fetched {  // one trip through the cache
    int rc = 0;  // SRACK_OK
    std::string err;
    CodePtr code;
    double compile_ms = 0.0;
    int how = 0;  // 0 memory, 1 disk, 2 compiled
};

// The current device's architecture without its feature suffixes ("gfx950"); gfx950 when the process has no device.
std::string device_arch();
// A kernel's name in the cache: architecture, compiler options, hiprtc version, the embedded device headers, the source.
std::string cache_key(const std::string& arch, const std::string& src);
// memory -> disk -> hiprtc.
Fetched fetch_code(const std::string& arch, const std::string& src);
// The loaded modules, by "<device>:" + cache_key.  find: the resident one (a memory hit) or null.  keep: `k` becomes the resident one
// unless another thread's got there first; returns the resident one.
std::shared_ptr<const JitKernel> kernel_cache_find(const std::string& kkey);
std::shared_ptr<const JitKernel> kernel_cache_keep(const std::string& kkey, std::shared_ptr<const JitKernel> k);
// The disk cache's directory: a path, "off", or nullptr for the default resolution (SRACK_KERNEL_CACHE_DIR, next to the library, ~/.cache).
int jit_cache_set_dir(const char* dir);
JitCacheStats jit_cache_stats();

}  // namespace srack
