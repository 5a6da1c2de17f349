// hiprtc helpers shared by the run-time compiled kernels (jit.cpp: per-plan VALU passes; hea_spec.cpp: per-plan MFMA
// passes): source hash, hiprtc compile for an offload arch (no GPU needed), and the on-disk code-object cache.
#pragma once

#include <hip/hiprtc.h>

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

namespace qfx {

inline std::string hex64(uint64_t h) {
  char b[17];
  std::snprintf(b, sizeof(b), "%016llx", (unsigned long long)h);
  return b;
}

inline uint64_t fnv1a(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char c : s) {
    h ^= c;
    h *= 1099511628211ull;
  }
  return h;
}

// "hiprtc<major>.<minor>": part of the code-object cache keys, so another compiler does not reuse an entry
inline std::string hiprtc_version_tag() {
  int major = 0, minor = 0;
  hiprtcVersion(&major, &minor);
  return "hiprtc" + std::to_string(major) + "." + std::to_string(minor);
}

inline bool file_exists(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0;
}

inline std::string read_text(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// Compile `src` for `arch` with `include_dir` on the include path.
inline std::vector<char> hiprtc_compile(const std::string& src, const std::string& include_dir, const std::string& arch) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "qfx_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    throw std::runtime_error("hiprtcCreateProgram failed");
  std::string a = "--offload-arch=" + arch, inc = "-I" + include_dir;
  const char* opts[] = {a.c_str(), inc.c_str(), "-O3", "-std=c++17"};
  hiprtcResult rc = hiprtcCompileProgram(prog, 4, opts);
  if (rc != HIPRTC_SUCCESS) {
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string log(ls, '\0');
    hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    throw std::runtime_error("hiprtc compile failed:\n" + log.substr(0, 4000));
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  std::vector<char> code(cs);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);
  return code;
}

// The cached code object of `key` (empty: none).
inline std::vector<char> cache_load(const std::string& cache_dir, const std::string& key) {
  std::vector<char> code;
  const std::string path = cache_dir + "/" + key + ".co";
  if (!cache_dir.empty() && file_exists(path)) {
    std::ifstream f(path, std::ios::binary);
    code.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  }
  return code;
}

// Store a code object and its source under `key`.  One temp file per process: the ranks of a node share the cache
// and may compile the same key at once; each renames a complete file of its own over the entry, so a reader never
// sees a partial code object.
inline void cache_store(const std::string& cache_dir, const std::string& key, const std::vector<char>& code,
                        const std::string& source) {
  if (cache_dir.empty()) return;
  mkdir(cache_dir.c_str(), 0755);
  const std::string path = cache_dir + "/" + key + ".co";
  const std::string tag = "." + std::to_string((long)getpid()) + ".tmp";
  const std::string tmp = path + tag;
  bool ok;
  {
    std::ofstream f(tmp, std::ios::binary);
    f.write(code.data(), (std::streamsize)code.size());
    ok = (bool)f;
  }
  if (ok) std::rename(tmp.c_str(), path.c_str());
  else std::remove(tmp.c_str());
  const std::string src = cache_dir + "/" + key + ".hip";
  {
    std::ofstream fs(src + tag);
    fs << source;
  }
  std::rename((src + tag).c_str(), src.c_str());
}

}  // namespace qfx
