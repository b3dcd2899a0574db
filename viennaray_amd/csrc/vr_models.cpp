// vr_models.cpp — particle models and source models registered at run time: the caller's text is compiled around the
// library's own kernel sources (vr_trace.hip and what it includes: the Makefile's MODEL_SRCS; a hipcc child, cached by content: build_code_object) and loaded as a code object.
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "vr_context.hpp"
#include "vr_particles.hpp"

// ---- run-time particle and source models -----------------------------------------------------------------------------------
static uint64_t fnv1a(uint64_t h, const void *data, size_t n) {
  const unsigned char *b = (const unsigned char *)data;
  for (size_t i = 0; i < n; ++i) {
    h ^= b[i];
    h *= 1099511628211ull;
  }
  return h;
}

// the files a run-time module is compiled from, blank separated: the Makefile's MODEL_SRCS, the one place that names them
#ifndef VR_MODEL_SRCS
#error "VR_MODEL_SRCS is not defined: build vr_models.cpp through the Makefile, which names a module's sources"
#endif

static bool slurp(const std::string &path, std::string &out) {
  std::ifstream f(path, std::ios::binary);
  if (!f)
    return false;
  std::ostringstream ss;
  ss << f.rdbuf();
  out = ss.str();
  return true;
}

// the kernel sources the library was built from: next to the library (in-tree layout viennaray_amd/csrc), or VR_CSRC_DIR
static std::string csrc_dir() {
  if (const char *e = std::getenv("VR_CSRC_DIR"))
    return e;
  Dl_info info;
  if (dladdr((const void *)&vr_version, &info) && info.dli_fname) {
    std::string p = info.dli_fname;
    const size_t k = p.find_last_of('/');
    return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/csrc";
  }
  return "csrc";
}

// POSIX cksum (CRC-32, polynomial 0x04C11DB7, the length appended) of a file's bytes: what the Makefile records of every
// kernel source at build time (VR_SRC_CKSUM) — a run-time model must be compiled from THOSE sources: its kernels take the
// library's TraceParams by value.
static uint32_t posix_cksum(const std::string &data) {
  static uint32_t table[256];
  static bool init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i << 24;
      for (int k = 0; k < 8; ++k)
        c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
      table[i] = c;
    }
    init = true;
  }
  uint32_t crc = 0;
  for (unsigned char b : data)
    crc = (crc << 8) ^ table[((crc >> 24) ^ b) & 0xFFu];
  for (size_t n = data.size(); n; n >>= 8)
    crc = (crc << 8) ^ table[((crc >> 24) ^ (n & 0xFFu)) & 0xFFu];
  return ~crc;
}

// the compiler's identity (`hipcc --version`, first lines), part of the cache key: a code object does not survive a
// toolchain upgrade
static std::string compiler_identity(const std::string &hipcc) {
  std::string out;
  if (hipcc.find('\'') != std::string::npos)
    return out;
  if (FILE *f = popen(("'" + hipcc + "' --version 2>/dev/null").c_str(), "r")) {
    char buf[256];
    while (out.size() < 2048 && std::fgets(buf, sizeof(buf), f))
      out += buf;
    pclose(f);
  }
  return out;
}

// What differs between the two kinds of run-time modules: the entry point's name in the messages, the name of the cache
// file, the file the caller's text is written to, and what the caller's text is called.
struct ModuleKind {
  const char *api;      // "vr_register_particle_model"
  const char *prefix;   // cache file: <prefix><hash>.hsaco
  const char *userFile; // the caller's text, next to the translation unit: <...><userFile>
  const char *fileMacro; // ... and the macro that names it to vr_trace.hip
  const char *noun;     // "model"
};

// One run-time module, from the caller's text to a code object in the cache: `h` is the hash of what the caller gave (the
// text and the options compiled into it) and goes on over the library's kernel sources — which must be the ones this
// library was built from — the compiler's identity and its flags; a code object of that name in the (checked) cache
// directory is reused, else the translation unit is written — `defines` (the kind's #define lines; the line that names
// the file with the caller's text is added here, as kind.fileMacro), the include of vr_trace.hip, `asserts` (the kind's
// static_asserts) and the layout check — a hipcc child compiles it under names of this process's own, and the code
// object moves into place atomically.  A compile error comes back as VR_E_INVALID with the compiler's error lines.  On
// success `hsaco` is the code object's path.
static int build_code_object(vr_context *c, const ModuleKind &kind, uint64_t h, const char *source, const std::string &defines,
                             const std::string &asserts, std::string &hsaco) {
  const std::string api = kind.api;
  const std::string csrc = csrc_dir();
  const std::string hipcc = std::getenv("VR_HIPCC") ? std::getenv("VR_HIPCC") : "/opt/rocm/bin/hipcc";
  const std::string ccFlags = " --genco --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-function";
  std::string cksums;
  std::istringstream names(VR_MODEL_SRCS);
  for (std::string fn; names >> fn;) {
    std::string text;
    if (!slurp(csrc + "/" + fn, text))
      return fail(c, VR_E_STATE, (api + ": kernel source not found: " + csrc + "/" + fn +
                                  " (the sources ship next to the library; VR_CSRC_DIR overrides)").c_str());
    h = fnv1a(h, text.data(), text.size());
    cksums += std::to_string(posix_cksum(text)) + "-";
  }
#ifdef VR_SRC_CKSUM
  // The kernels of the module take the library's TraceParams by value and read the LDS frame the host fills: sources that
  // are not the ones this library was built from (an edited checkout without a rebuild, a wrong VR_CSRC_DIR, an installed
  // library next to a newer tree) would end in a GPU memory fault, not in an error code.  Refused here.
  if (cksums != VR_SRC_CKSUM)
    return fail(c, VR_E_STATE, (api + ": the kernel sources in " + csrc + " are not the ones this library was built "
                                "from (checksums " + cksums + " against " VR_SRC_CKSUM "): rebuild the library, or point VR_CSRC_DIR at its sources").c_str());
#endif
  { // (a code object does not survive a change of the compiler or of its flags)
    const std::string id = compiler_identity(hipcc) + ccFlags;
    h = fnv1a(h, id.data(), id.size());
  }
  // The cache holds code that hipModuleLoad will run: a directory of the caller's own, mode 0700, and checked — a
  // predictable name under /tmp that another local user created first could hold a planted code object.
  std::string cache;
  if (const char *e = std::getenv("VR_CACHE_DIR"))
    cache = e;
  else if (const char *x = std::getenv("XDG_CACHE_HOME"); x && *x)
    cache = std::string(x) + "/viennaray_amd";
  else if (const char *hm = std::getenv("HOME"); hm && *hm && std::string(hm) != "/") {
    (void)mkdir((std::string(hm) + "/.cache").c_str(), 0700);
    cache = std::string(hm) + "/.cache/viennaray_amd";
  } else
    cache = "/tmp/viennaray_amd_cache_" + std::to_string((unsigned)getuid());
  (void)mkdir(cache.c_str(), 0700);
  {
    struct stat ds;
    if (lstat(cache.c_str(), &ds) != 0 || !S_ISDIR(ds.st_mode) || ds.st_uid != getuid() || (ds.st_mode & 077) != 0)
      return fail(c, VR_E_STATE, (api + ": the code-object cache " + cache + " must be a directory (no symbolic link) "
                                  "owned by this user with mode 0700 - refused; set VR_CACHE_DIR to a private directory").c_str());
  }
  char hex[32];
  std::snprintf(hex, sizeof(hex), "%016llx", (unsigned long long)h);
  const std::string base = cache + "/" + kind.prefix + hex;
  hsaco = base + ".hsaco";
  struct stat st;
  if (stat(hsaco.c_str(), &st) != 0 || st.st_size == 0) {
    // every file of this compilation under a name of this process's own (several ranks register the same model on a cold
    // cache at once); the code object then moves into place atomically
    const std::string mine = base + ".p" + std::to_string((int)getpid());
    const std::string tmp = mine + ".hsaco";
    { std::ofstream f(mine + kind.userFile); f << source << "\n"; }
    {
      std::ofstream f(mine + ".hip");
      f << "// generated by " << api << "\n" << defines << "#define " << kind.fileMacro << " \"" << mine << kind.userFile
        << "\"\n#include <cstddef>\n#include \"" << csrc << "/vr_trace.hip\"\n" << asserts;
      // the launch parameters and the LDS frame as THIS library lays them out
      f << "static_assert(sizeof(vr::TraceParams) == " << sizeof(TraceParams) << " && offsetof(vr::TraceParams, globalVec) == "
        << offsetof(TraceParams, globalVec) << " && offsetof(vr::TraceParams, counters) == " << offsetof(TraceParams, counters)
        << " && offsetof(vr::TraceParams, pqMargin) == " << offsetof(TraceParams, pqMargin) << " && vr::VR_WALL_TABLE == "
        << VR_WALL_TABLE << ", \"vr::TraceParams / the launch frame differ from the loaded library's: these kernel sources are not its own\");\n";
    }
    auto quoted = [](const std::string &path) { return "'" + path + "'"; }; // (paths with blanks; a quote in a path is refused below)
    if ((cache + csrc + hipcc).find('\'') != std::string::npos)
      return fail(c, VR_E_INVALID, (api + ": the cache / source directory must not contain a quote character").c_str());
    const std::string cmd = quoted(hipcc) + ccFlags + " -I" + quoted(csrc) + " " + quoted(mine + ".hip") + " -o " + quoted(tmp) + " > " +
                            quoted(mine + ".log") + " 2>&1";
    const int rc = std::system(cmd.c_str());
    (void)unlink((mine + ".hip").c_str());
    (void)unlink((mine + kind.userFile).c_str());
    if (rc != 0) {
      std::string all, log;
      (void)slurp(mine + ".log", all);
      (void)std::rename((mine + ".log").c_str(), (base + ".log").c_str()); // (kept for the caller to read)
      { // the compiler's error lines (and the source line under each), not the tail of its output
        std::istringstream in(all);
        std::string line;
        int keep = 0;
        while (std::getline(in, line) && log.size() < 1500) {
          if (line.find("error") != std::string::npos)
            keep = 3;
          if (keep-- > 0)
            log += line + "\n";
        }
        if (log.empty())
          log = all.size() > 1500 ? all.substr(all.size() - 1500) : all;
      }
      (void)unlink(tmp.c_str());
      return fail(c, VR_E_INVALID, (api + ": the " + kind.noun + " did not compile (" + base + ".log):\n" + log).c_str());
    }
    (void)unlink((mine + ".log").c_str());
    if (std::rename(tmp.c_str(), hsaco.c_str()) != 0)
      return fail(c, VR_E_STATE, (api + ": cannot write the code object cache").c_str());
  }
  return VR_OK;
}

// A particle model's code object: the extended trace kernels around the caller's text, or (stats) its twin with the flux
// statistics compiled in (VR_USER_FLUX_STATS, vr_modules.hpp) — a code object and a cache key of its own.
static int build_particle_module(vr_context *c, const char *source, int numData, int numState, bool full, bool stats, std::string &hsaco) {
  uint64_t h = 1469598103934665603ull;
  h = fnv1a(h, source, std::strlen(source));
  h = fnv1a(h, &numData, sizeof(numData));
  h = fnv1a(h, &full, sizeof(full));
  h = fnv1a(h, &numState, sizeof(numState));
  if (stats) // (statistics off: the key the module always had)
    h = fnv1a(h, "flux-statistics", 15);
  static const ModuleKind kind{"vr_register_particle_model", "model_", "_model.hpp", "VR_USER_MODEL_FILE", "model"};
  return build_code_object(c, kind, h, source,
                           "#define VR_USER_MODULE 1\n#define VR_USER_NUM_DATA " + std::to_string(numData) +
                               "\n#define VR_USER_NUM_STATE " + std::to_string(numState) + "\n" +
                               (stats ? "#define VR_USER_FLUX_STATS 1\n" : ""),
                           std::string("static_assert(vr::VrUserModel::kNeedsFull == ") + (full ? "true" : "false") +
                               ", \"kNeedsFull differs from the VR_MODEL_NEEDS_FULL flag given at registration\");\n",
                           hsaco);
}

// the trace kernels of a loaded particle module — the catalogue's KERNELS_MODULE set (vr_types.hpp) under the module's
// particle id — by their mangled names (key: module_kernel_key, vr_types.hpp)
static int find_trace_kernels(vr_context *c, hipModule_t module, bool full, bool stats, std::map<int, hipFunction_t> &kernels) {
  const int P = stats ? (full ? (int)P_EXT_FULL_STATS : (int)P_EXT_STATS) : (full ? (int)P_EXT_FULL : (int)P_EXT);
  for (int D = 2; D <= 3; ++D)
    for (int geo = 0; geo <= 1; ++geo)
      for (int mode = 0; mode < VR_NUM_MODES; ++mode) {
        if (!trace_kernel_exists(KERNELS_MODULE, D, geo, P, mode))
          continue;
        char sym[128];
        std::snprintf(sym, sizeof(sym), "_ZN2vr12trace_kernelILi%dELi%dELi%dELi%dEEEvNS_11TraceParamsE", D, geo, P, mode);
        hipFunction_t f = nullptr;
        if (hipModuleGetFunction(&f, module, sym) != hipSuccess || !f)
          return fail(c, VR_E_STATE, (std::string("vr_register_particle_model: kernel missing from the code object: ") + sym).c_str());
        kernels[module_kernel_key(D, geo, mode)] = f;
      }
  return VR_OK;
}

namespace vr {
// flux statistics: the model's twin module, built (or found in the cache) and loaded when a statistics-on apply first needs it
int ensure_stats_module(vr_context *c, UserModel &um) {
  if (um.statsModule)
    return VR_OK;
  VR_HIP(c, hipSetDevice(c->device));
  std::string hsaco;
  VR_TRY(build_particle_module(c, um.source.c_str(), um.numData, um.numState, um.needsFull, true, hsaco));
  hipModule_t m = nullptr;
  VR_HIP(c, hipModuleLoad(&m, hsaco.c_str()));
  std::map<int, hipFunction_t> kernels;
  const int r = find_trace_kernels(c, m, um.needsFull, true, kernels);
  if (r != VR_OK) {
    (void)hipModuleUnload(m);
    return r;
  }
  um.statsModule = m;
  um.statsKernels = std::move(kernels);
  return VR_OK;
}
} // namespace vr

extern "C" {

// The reference's GPU path registers user callables per particle at run time (gpu/raygCallableConfig.hpp:7-18: OptiX
// direct callables named in the particle).  Here the caller hands over the SOURCE of a model — `struct VrUserModel` with
// the registry's shape (vr_particles.hpp: sticking / reflect / collide, kNumData, kNeedsFull), usually a few lines on top of
// one of the built-in models — and the library compiles the extended trace kernels around it for gfx950 (hipcc --genco,
// cached by content) and loads them.  The returned kind goes into vr_particle::kind like a built-in one.
int vr_register_particle_model(vr_context *c, const char *name, const char *source, int numData, int flags, int32_t *kindOut) {
  return vr_register_particle_model_ex(c, name, source, numData, 0, flags, kindOut);
}

// ... with per-ray state: numState = VrUserModel::kStateWords (0 .. 4; > 0: a stateful model, vr_particles.hpp — it runs in
// the P_EXT_FULL kernels, so VR_MODEL_NEEDS_FULL is implied, and its module holds a generator of its own)
int vr_register_particle_model_ex(vr_context *c, const char *name, const char *source, int numData, int numState, int flags,
                                  int32_t *kindOut) {
  if (!c || !source || !kindOut || numData < 1 || numData > VR_MAX_LABELS)
    return fail(c, VR_E_INVALID, "vr_register_particle_model: bad argument (1 .. 4 data labels)");
  if (numState < 0 || numState > VR_MAX_STATE_WORDS)
    return fail(c, VR_E_INVALID, "vr_register_particle_model_ex: numState (the model's kStateWords) must be 0 .. 4");
  VR_HIP(c, hipSetDevice(c->device));
  const bool full = (flags & VR_MODEL_NEEDS_FULL) != 0 || numState > 0;
  std::string hsaco;
  VR_TRY(build_particle_module(c, source, numData, numState, full, false, hsaco));
  UserModel um;
  um.name = name ? name : "";
  um.source = source;
  um.numData = numData;
  um.needsFull = full;
  um.numState = numState;
  VR_HIP(c, hipModuleLoad(&um.module, hsaco.c_str()));
  if (numState > 0)
    for (int D = 2; D <= 3; ++D) {
      char sym[128];
      std::snprintf(sym, sizeof(sym), "_ZN2vr16gen_state_kernelILi%dENS_11VrUserModelEEEvNS_11TraceParamsE", D);
      if (hipModuleGetFunction(&um.gen[D - 2], um.module, sym) != hipSuccess || !um.gen[D - 2]) {
        (void)hipModuleUnload(um.module);
        return fail(c, VR_E_STATE, (std::string("vr_register_particle_model: kernel missing from the code object: ") + sym).c_str());
      }
    }
  { // the rows its log_data hook writes (kLogRows), from the module itself
    hipDeviceptr_t sym = nullptr;
    size_t bytes = 0;
    int32_t rows = 0;
    if (hipModuleGetGlobal(&sym, &bytes, um.module, "vr_user_log_rows") != hipSuccess || bytes != sizeof(rows) ||
        hipMemcpy(&rows, (const void *)sym, sizeof(rows), hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipModuleUnload(um.module);
      return fail(c, VR_E_STATE, "vr_register_particle_model: symbol missing from the code object: vr_user_log_rows");
    }
    um.logRows = rows;
  }
  if (const int r = find_trace_kernels(c, um.module, full, false, um.kernels); r != VR_OK) {
    (void)hipModuleUnload(um.module);
    return r;
  }
  c->userModels.push_back(std::move(um));
  *kindOut = VR_PARTICLE_USER_BASE + (int32_t)c->userModels.size() - 1;
  return VR_OK;
}

// A SOURCE model registered at run time: the reference's Source<NumericType> (raySource.hpp:10-19) as device code.  `source`
// is HIP text that defines `struct VrUserSource` (vr_modules.hpp, the source-module section, says what it looks like); the
// library compiles the generator around it for gfx950 — no trace kernel: a fraction of a particle module's compile time —
// caches the code object by content and loads it (a text this context has registered already gives its id again: nothing
// is loaded twice).  flags: VR_SOURCE_HAS_WEIGHT exactly when the model's kHasWeight is true.
// The returned id goes into vr_set_source_model.  A text that does not compile: VR_E_INVALID with the compiler's error lines.
int vr_register_source_model(vr_context *c, const char *name, const char *source, int flags, int32_t *sourceId) {
  if (!c || !source || !sourceId || (flags & ~VR_SOURCE_HAS_WEIGHT) != 0)
    return fail(c, VR_E_INVALID, "vr_register_source_model: bad argument (flags: 0 or VR_SOURCE_HAS_WEIGHT)");
  VR_HIP(c, hipSetDevice(c->device));
  const bool hasWeight = (flags & VR_SOURCE_HAS_WEIGHT) != 0;
  uint64_t h = 1469598103934665603ull;
  h = fnv1a(h, source, std::strlen(source));
  h = fnv1a(h, &hasWeight, sizeof(hasWeight));
  static const ModuleKind kind{"vr_register_source_model", "source_", "_source.hpp", "VR_USER_SOURCE_FILE", "source model"};
  std::string hsaco;
  VR_TRY(build_code_object(c, kind, h, source,
                           std::string("#define VR_USER_MODULE 1\n#define VR_USER_SOURCE_MODULE 1\n#define VR_USER_SOURCE_HAS_WEIGHT ") +
                               (hasWeight ? "1\n" : "0\n"),
                           // (the generator takes the context by value as well)
                           "static_assert(sizeof(vr::SourceCtx) == " + std::to_string(sizeof(SourceCtx)) +
                               " && offsetof(vr::SourceCtx, table) == " + std::to_string(offsetof(SourceCtx, table)) +
                               " && offsetof(vr::SourceCtx, params) == " + std::to_string(offsetof(SourceCtx, params)) +
                               ", \"vr::SourceCtx differs from the loaded library's: these kernel sources are not its own\");\n",
                           hsaco));
  // the same text with the same flag is the same code object: registered once per context, however often it is asked for
  for (size_t k = 0; k < c->sourceModels.size(); ++k)
    if (c->sourceModels[k].codeObject == hsaco) {
      *sourceId = (int32_t)k;
      return VR_OK;
    }
  SourceModel sm;
  sm.name = name ? name : "";
  sm.codeObject = hsaco;
  sm.hasWeight = hasWeight;
  VR_HIP(c, hipModuleLoad(&sm.module, hsaco.c_str()));
  auto missing = [&](const char *sym) {
    (void)hipModuleUnload(sm.module);
    return fail(c, VR_E_STATE, (std::string("vr_register_source_model: kernel missing from the code object: ") + sym).c_str());
  };
  for (int D = 2; D <= 3; ++D) {
    char sym[160];
    for (int keep = 0; keep <= 1; ++keep) {
      std::snprintf(sym, sizeof(sym), "_ZN2vr22gen_user_source_kernelILi%dELb%dEEEvNS_11TraceParamsENS_9SourceCtxE", D, keep);
      if (hipModuleGetFunction(&sm.gen[D - 2][keep], sm.module, sym) != hipSuccess || !sm.gen[D - 2][keep])
        return missing(sym);
    }
    std::snprintf(sym, sizeof(sym), "_ZN2vr24debug_user_source_kernelILi%dEEEvNS_11TraceParamsENS_9SourceCtxEPfS3_S3_Pj", D);
    if (hipModuleGetFunction(&sm.debug[D - 2], sm.module, sym) != hipSuccess || !sm.debug[D - 2])
      return missing(sym);
  }
  c->sourceModels.push_back(std::move(sm));
  *sourceId = (int32_t)c->sourceModels.size() - 1;
  return VR_OK;
}

int vr_get_model_log_rows(const vr_context *c, int32_t kind, int32_t *rows) {
  if (!c || !rows)
    return VR_E_INVALID;
  const int32_t u = kind - VR_PARTICLE_USER_BASE;
  *rows = (u >= 0 && u < (int32_t)c->userModels.size()) ? c->userModels[u].logRows : 0; // (the built-in models log nothing)
  return VR_OK;
}

} // extern "C"
