// codecad_amd/csrc/tape_build.hip -- host only, no kernel: a tape's own kernels from the decoded program to the handle.
// The program is unrolled into source (specialise.hpp), compiled with hipRTC -- with a precompiled header where the
// installation has a clang to make one --, kept in an on-disk cache and loaded into the handle (tape_handle.hpp), where
// hip_util.hip finds the kernels to launch.  Also the listings of a tape's programs and source.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include <dirent.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

extern char** environ;

#include "host.hpp"
#include "tape_handle.hpp"

using sdf::Rec;

namespace {

std::string generate_source(const hu_tape_s* t, sdf::SpecMeta* meta = nullptr)
{
    return sdf::specialised_source(t->program, meta);
}

// ---- specialised code objects: hipRTC build + optional on-disk cache ------------------------
// What hu_tape_specialize needs from a build: the code object and, per kernel of kSpecKernelNames, its
// lowered (mangled) name.  With a cache directory the image is stored under a key made of everything the
// build depends on -- generated source, the op library headers it includes, the compiler options, the
// hipRTC / HIP versions -- so a later process (or a later tape with the same program) loads it in
// milliseconds instead of compiling for seconds.  The cache is best effort: unreadable, truncated or
// foreign files are ignored and rebuilt, an unwritable directory is not an error.
struct SpecImage {
    std::vector<std::string> lowered;
    std::vector<char> code;
};

const char* const kSpecHeaders[] = {"kernels.hpp", "interp.hpp", "tape_format.hpp", "sdf_math.hpp"};
const char kSpecMagic[8] = {'H', 'U', 'S', 'P', 'E', 'C', '1', 0};

uint64_t fnv1a(uint64_t h, const void* data, size_t n)
{
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

bool read_file(const std::string& path, std::string& out)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    const bool ok = !std::ferror(f);
    std::fclose(f);
    return ok;
}

// A source above this size is built with -O1: what takes the time in a kernel of 200 KB is code generation, the straight-line
// code the generator writes leaves the optimiser little to do, and -O1 spends a third less on it for the same kernels
// (planetary, 855 KB of source, MI355X box: first per-tape launch 4.0 -> 2.6 s after upload, all kernels 4.4 -> 2.9 s; C4 0.383
// ms, its 256^3 grids 0.19 / 0.57 ms, C3 and C5 at -O1: all unchanged; the parity tests pass either way).  Small sources gain
// nothing (sponge(4), 80 KB: 0.26 s either way) and keep -O3.  HU_RTC_BIG_KB: the threshold in KiB (default 256, 0: never).
bool spec_source_is_big(size_t bytes)
{
    static const size_t limit = [] { const char* e = getenv("HU_RTC_BIG_KB"); const long v = e ? atol(e) : 256; return (size_t)(v > 0 ? v : 0) * 1024u; }();
    return limit != 0 && bytes > limit;
}

std::vector<std::string> spec_options(const char* include_dir, bool big = false)
{
    // same numerical contract as the ahead-of-time build: no contraction, IEEE sqrt/divide (HIP default)
    std::vector<std::string> opts = {"--offload-arch=gfx950", big ? "-O1" : "-O3", "-std=c++17", "-ffp-contract=off",
                                     std::string("-I") + include_dir};
    if (const char* e = getenv("HU_RTC_FLAGS")) {  // extra compiler options, for tuning experiments
        std::istringstream in(e);
        for (std::string w; in >> w;) opts.push_back(w);
    }
    return opts;
}

// Two independent 64-bit hashes over everything the build depends on; false if a header cannot be read
// (then nothing is cached).
bool spec_cache_key(const std::string& src, const char* include_dir, const std::vector<std::string>& opts, uint32_t groups,
                           uint64_t key[2])
{
    uint64_t h[2] = {0xcbf29ce484222325ull, 0x84222325cbf29ce4ull};
    auto mix = [&](const void* p, size_t n) {
        const uint64_t len = n;
        for (int i = 0; i < 2; ++i) {
            h[i] = fnv1a(h[i], &len, sizeof len);
            h[i] = fnv1a(h[i], p, n);
        }
    };
    int version[3] = {0, 0, HIP_VERSION};
    (void)hiprtcVersion(&version[0], &version[1]);
    mix(version, sizeof version);
    mix(src.data(), src.size());
    for (size_t i = 0; i < opts.size(); ++i)  // the include path itself does not matter, the headers' bytes do
        if (opts[i].compare(0, 2, "-I") != 0) mix(opts[i].data(), opts[i].size());
    for (int i = 0; i < kSpecKernelCount; ++i)   // the kernels of this build: a build of other families is another file
        if (kSpecGroupOf[i] & groups) mix(kSpecKernelNames[i], std::strlen(kSpecKernelNames[i]));
    std::string text;
    for (const char* name : kSpecHeaders) {
        if (!read_file(std::string(include_dir) + "/" + name, text)) return false;
        mix(text.data(), text.size());
    }
    key[0] = h[0];
    key[1] = h[1] ^ 0x9e3779b97f4a7c15ull;
    return true;
}

std::string spec_cache_path(const char* cache_dir, const uint64_t key[2])
{
    char name[64];
    std::snprintf(name, sizeof name, "/%016llx%016llx.huspec", (unsigned long long)key[0], (unsigned long long)key[1]);
    return std::string(cache_dir) + name;
}

uint32_t spec_kernels_in(uint32_t groups)
{
    uint32_t n = 0;
    for (int i = 0; i < kSpecKernelCount; ++i) n += (kSpecGroupOf[i] & groups) ? 1u : 0u;
    return n;
}

bool spec_cache_load(const std::string& path, const uint64_t key[2], uint32_t groups, SpecImage& img)
{
    std::string blob;
    if (!read_file(path, blob)) return false;
    size_t pos = 0;
    auto take = [&](void* dst, size_t n) {
        if (blob.size() - pos < n) return false;
        std::memcpy(dst, blob.data() + pos, n);
        pos += n;
        return true;
    };
    char magic[8];
    uint64_t k[2], code_size, sum;
    uint32_t names;
    if (!take(magic, 8) || std::memcmp(magic, kSpecMagic, 8) != 0 || !take(k, 16) || k[0] != key[0] || k[1] != key[1] ||
        !take(&names, 4) || names != spec_kernels_in(groups))
        return false;
    img.lowered.clear();
    for (uint32_t i = 0; i < names; ++i) {
        uint32_t len;
        if (!take(&len, 4) || len == 0 || len > 4096 || blob.size() - pos < len) return false;
        img.lowered.emplace_back(blob.data() + pos, len);
        pos += len;
    }
    if (!take(&code_size, 8) || code_size == 0 || blob.size() - pos != code_size + 8) return false;
    img.code.assign(blob.begin() + pos, blob.begin() + pos + code_size);
    pos += code_size;
    return take(&sum, 8) && sum == fnv1a(0xcbf29ce484222325ull, blob.data(), blob.size() - 8);  // covers names and code
}

void spec_cache_store(const char* cache_dir, const std::string& path, const uint64_t key[2], const SpecImage& img)
{
    (void)mkdir(cache_dir, 0700);  // one level; the caller creates parents
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
    std::string blob(kSpecMagic, 8);
    auto put = [&](const void* p, size_t n) { blob.append(static_cast<const char*>(p), n); };
    put(key, 16);
    const uint32_t names = (uint32_t)img.lowered.size();
    put(&names, 4);
    for (const std::string& n : img.lowered) {
        const uint32_t len = (uint32_t)n.size();
        put(&len, 4);
        put(n.data(), len);
    }
    const uint64_t code_size = img.code.size();
    put(&code_size, 8);
    put(img.code.data(), img.code.size());
    const uint64_t sum = fnv1a(0xcbf29ce484222325ull, blob.data(), blob.size());
    put(&sum, 8);
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return;
    bool ok = std::fwrite(blob.data(), 1, blob.size(), f) == blob.size();
    ok = (std::fclose(f) == 0) && ok;
    if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) (void)std::remove(tmp.c_str());  // atomic publish
}

// Keep the cache bounded: beyond kSpecCacheFiles entries the oldest (by modification time) are removed.
constexpr size_t kSpecCacheFiles = 8192;    // (up to nineteen per tape)
void spec_cache_prune(const char* cache_dir)
{
    DIR* d = opendir(cache_dir);
    if (!d) return;
    std::vector<std::pair<int64_t, std::string>> files;
    while (const dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name.size() < 8 || name.compare(name.size() - 7, 7, ".huspec") != 0) continue;
        struct stat st;
        const std::string path = std::string(cache_dir) + "/" + name;
        if (stat(path.c_str(), &st) == 0) files.emplace_back((int64_t)st.st_mtime, path);
    }
    closedir(d);
    if (files.size() <= kSpecCacheFiles) return;
    std::sort(files.begin(), files.end());
    for (size_t i = 0; i + kSpecCacheFiles * 3 / 4 < files.size(); ++i) (void)std::remove(files[i].second.c_str());
}

// ---- a precompiled header for the per-tape builds --------------------------------------------------------------------
// A per-tape build parses the same ~16 000 lines every time -- hipRTC's own runtime header (13 000) and the op library
// (kernels.hpp and what it includes) -- before it sees the first line that depends on the tape: a quarter of a family's
// build, and most of a single small kernel's.  hipRTC hands its options to clang, `-include-pch` among them; what it cannot
// do is WRITE one.  So the header is made once per (cache directory, op library, hipRTC installation) by the clang++ that
// sits next to the hipRTC in use (<lib>/llvm/bin/clang++: same compiler, or the file is refused and the build goes on
// without -- as it does when there is no such clang, e.g. under the hipRTC a PyTorch wheel brings along), from hipRTC's
// runtime header (libhiprtc-builtins.so exports its text) and with the options hipRTC itself passes.  Best effort all the
// way: no clang, no builtins library, a directory that cannot be written, a header another process is just making, a file
// clang refuses -- the build runs as before.  HU_RTC_PCH=0 switches it off, HU_CLANG names the compiler.
std::atomic<bool> g_pch_refused{false};          // the compiler in this process refused a header once: do not offer it again
std::atomic<bool> g_pch_beside_refused{false};   // ... the one beside the library (then: one of its own, in the cache directory)
std::mutex g_pch_mutex;                          // builds may run on several threads of a process (buffer.py, servers off)

std::string dir_of(const std::string& path)
{
    const size_t cut = path.rfind('/');
    return cut == std::string::npos ? std::string(".") : path.substr(0, cut);
}

bool run_and_wait(const std::vector<std::string>& argv)
{
    std::vector<char*> av;
    for (const std::string& a : argv) av.push_back(const_cast<char*>(a.c_str()));
    av.push_back(nullptr);
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_addopen(&fa, 0, "/dev/null", O_RDONLY, 0);
    posix_spawn_file_actions_addopen(&fa, 1, "/dev/null", O_WRONLY, 0);   // (a compile server talks on its stdout)
    posix_spawn_file_actions_addopen(&fa, 2, "/dev/null", O_WRONLY, 0);
    pid_t pid = 0;
    const int rc = posix_spawn(&pid, av[0], &fa, nullptr, av.data(), environ);
    posix_spawn_file_actions_destroy(&fa);
    if (rc != 0) return false;
    int status = 0;
    while (waitpid(pid, &status, 0) < 0)
        if (errno != EINTR) return false;
    return WIFEXITED(status) && WEXITSTATUS(status) == 0;
}

// -> the path of a usable precompiled header, or "" (then the build runs without one): the one the library's build left
// next to the library (<directory of libhip_util.so>/pch, builder.py), else the one in `dir` (NULL: none), made now if need be
std::string spec_pch(const char* include_dir, const char* dir, const std::vector<std::string>& options, bool only_in_dir = false)
{
    static const bool off = [] { const char* e = getenv("HU_RTC_PCH"); return e && e[0] == '0'; }();
    if (off || g_pch_refused) return "";
    Dl_info where{};
    if (!dladdr(reinterpret_cast<const void*>(&hiprtcCompileProgram), &where) || !where.dli_fname) return "";
    const std::string lib_dir = dir_of(where.dli_fname);
    std::string clang;
    if (const char* e = getenv("HU_CLANG")) clang = e;
    else
        for (const char* rel : {"/llvm/bin/clang++", "/../llvm/bin/clang++", "/../lib/llvm/bin/clang++"})
            if (clang.empty() && access((lib_dir + rel).c_str(), X_OK) == 0) clang = lib_dir + rel;
    if (clang.empty() || access(clang.c_str(), X_OK) != 0) return "";
    // its name: everything it depends on
    uint64_t h = 0xcbf29ce484222325ull;
    int version[3] = {0, 0, HIP_VERSION};
    (void)hiprtcVersion(&version[0], &version[1]);
    h = fnv1a(h, version, sizeof version);
    h = fnv1a(h, lib_dir.data(), lib_dir.size());
    h = fnv1a(h, clang.data(), clang.size());
    for (const std::string& o : options)
        if (o.compare(0, 2, "-I") != 0) h = fnv1a(h, o.data(), o.size() + 1);   // (not the include path: the headers' bytes)
    std::string text;
    for (const char* name : kSpecHeaders) {
        if (!read_file(std::string(include_dir) + "/" + name, text)) return "";
        h = fnv1a(h, text.data(), text.size());
    }
    char hex[32];
    std::snprintf(hex, sizeof hex, "%016llx", (unsigned long long)h);
    if (!only_in_dir) {
        Dl_info self{};
        if (dladdr(reinterpret_cast<const void*>(&hu_last_error), &self) && self.dli_fname) {
            const std::string beside = dir_of(self.dli_fname) + "/pch/pch_" + hex + ".pch";
            if (access(beside.c_str(), R_OK) == 0) return beside;
        }
    }
    if (!dir || !*dir) return "";
    const std::string base = std::string(dir) + "/pch_" + hex, pch = base + ".pch";
    if (access(pch.c_str(), R_OK) == 0) return pch;
    std::lock_guard<std::mutex> one_at_a_time(g_pch_mutex);
    if (access(pch.c_str(), R_OK) == 0) return pch;      // (another thread made it meanwhile)
    static std::vector<std::string> tried;     // one attempt per process and name
    if (std::find(tried.begin(), tried.end(), base) != tried.end()) return "";
    tried.push_back(base);
    // one process makes it; the others carry on without it meanwhile (a lock left behind by a crash expires)
    const std::string lock = base + ".lock";
    (void)mkdir(dir, 0700);
    int fd = open(lock.c_str(), O_CREAT | O_EXCL | O_WRONLY, 0600);
    if (fd < 0) {
        struct stat st;
        if (stat(lock.c_str(), &st) == 0 && time(nullptr) - st.st_mtime > 120) (void)unlink(lock.c_str());
        return "";
    }
    close(fd);
    bool ok = false;
    do {
        // hipRTC's runtime header, the text its own builds start from
        void* builtins = nullptr;
        for (const std::string& name : {lib_dir + "/libhiprtc-builtins.so", std::string("libhiprtc-builtins.so." + std::to_string(version[0])),
                                        std::string("libhiprtc-builtins.so")})
            if (!builtins) builtins = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!builtins) break;
        const char* header = static_cast<const char*>(dlsym(builtins, "__hipRTC_header"));
        const unsigned* header_size = static_cast<const unsigned*>(dlsym(builtins, "__hipRTC_header_size"));
        if (!header || !header_size || *header_size == 0) break;
        size_t n = *header_size;
        while (n > 0 && header[n - 1] == 0) --n;
        const std::string inc = base + "_include";
        (void)mkdir(inc.c_str(), 0755);
        const std::string tmp_tag = ".tmp" + std::to_string((long)getpid());
        FILE* f = std::fopen((inc + "/hiprtc_runtime.h" + tmp_tag).c_str(), "wb");
        if (!f) break;
        const bool wrote = std::fwrite(header, 1, n, f) == n;
        if ((std::fclose(f) != 0) || !wrote || std::rename((inc + "/hiprtc_runtime.h" + tmp_tag).c_str(), (inc + "/hiprtc_runtime.h").c_str()) != 0) break;
        f = std::fopen((base + ".hip").c_str(), "wb");
        if (!f) break;
        std::fputs("#include \"kernels.hpp\"\n", f);
        if (std::fclose(f) != 0) break;
        // the options hipRTC passes for a HIP source (amd_comgr: COMPILE_SOURCE_TO_RELOCATABLE), then ours
        const std::string v = std::to_string(HIP_VERSION_MAJOR) + "." + std::to_string(HIP_VERSION_MINOR) + "." + std::to_string(HIP_VERSION_PATCH);
        std::vector<std::string> argv = {clang, "-c", "-fhip-emit-relocatable", "-mllvm", "-amdgpu-internalize-symbols", "-I", inc, "-O3", "-x", "hip",
                                         "--offload-device-only", "--hip-version=" + v, "-DHIP_VERSION_MAJOR=" + std::to_string(HIP_VERSION_MAJOR),
                                         "-DHIP_VERSION_MINOR=" + std::to_string(HIP_VERSION_MINOR), "-DHIP_VERSION_PATCH=" + std::to_string(HIP_VERSION_PATCH),
                                         "-Wno-gnu-line-marker", "-Wno-missing-prototypes", "-D__HIPCC_RTC__", "-nogpuinc", "-include", "hiprtc_runtime.h"};
        for (const std::string& o : options) argv.push_back(o);
        for (const char* o : {"-Xclang", "-emit-pch", "-Xclang", "-fno-pch-timestamp", "-o"}) argv.push_back(o);
        argv.push_back(pch + tmp_tag);
        argv.push_back(base + ".hip");
        if (!run_and_wait(argv)) { (void)std::remove((pch + tmp_tag).c_str()); break; }
        ok = std::rename((pch + tmp_tag).c_str(), pch.c_str()) == 0;
    } while (false);
    (void)unlink(lock.c_str());
    return ok ? pch : "";
}

// Compile `src` with hipRTC (needs no device) into an image.
int compile_specialised(const std::string& src, const std::vector<std::string>& options, uint32_t groups, SpecImage& img)
{
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "tape_specialised.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return hu_fail(HU_ERR_UNSUPPORTED, "hiprtcCreateProgram failed");
    for (int i = 0; i < kSpecKernelCount; ++i)
        if (kSpecGroupOf[i] & groups) (void)hiprtcAddNameExpression(prog, kSpecKernelNames[i]);
    std::vector<const char*> opts;
    for (const std::string& w : options) opts.push_back(w.c_str());
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string log;
        if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
            log.resize(n);
            (void)hiprtcGetProgramLog(prog, &log[0]);
        }
        (void)hiprtcDestroyProgram(&prog);
        return hu_fail(HU_ERR_UNSUPPORTED, std::string("hipRTC compile failed: ") + hiprtcGetErrorString(rc) + "\n" + log.substr(0, 4000));
    }
    size_t size = 0;
    (void)hiprtcGetCodeSize(prog, &size);
    img.code.resize(size);
    (void)hiprtcGetCode(prog, img.code.data());
    img.lowered.clear();
    for (int i = 0; i < kSpecKernelCount; ++i) {
        if (!(kSpecGroupOf[i] & groups)) continue;
        const char* name = kSpecKernelNames[i];
        const char* lowered = nullptr;
        if (hiprtcGetLoweredName(prog, name, &lowered) != HIPRTC_SUCCESS || !lowered) {
            (void)hiprtcDestroyProgram(&prog);
            return hu_fail(HU_ERR_UNSUPPORTED, std::string("kernel missing from the specialised module: ") + name);
        }
        img.lowered.emplace_back(lowered);
    }
    (void)hiprtcDestroyProgram(&prog);
    return HU_OK;
}

// The image of `src`: from the cache when it is there, else built (and stored).  With only_if_cached a miss
// leaves img.code empty and is not an error.
int specialised_image(const std::string& src, const char* include_dir, const char* cache_dir, bool only_if_cached, uint32_t groups,
                             SpecImage& img, int* from_cache, bool replace_cached = false)
{
    if (from_cache) *from_cache = 0;
    img.code.clear();
    const std::vector<std::string> options = spec_options(include_dir, spec_source_is_big(src.size()));
    uint64_t key[2];
    std::string path;
    const bool cached = cache_dir && *cache_dir && spec_cache_key(src, include_dir, options, groups, key);
    if (cached) {
        path = spec_cache_path(cache_dir, key);
        if (!replace_cached && spec_cache_load(path, key, groups, img)) {
            if (from_cache) *from_cache = 1;
            return HU_OK;
        }
        img.code.clear();
    }
    if (only_if_cached) return HU_OK;
    int rc = HU_ERR_UNSUPPORTED;
    for (int attempt = 0; attempt < 2 && rc != HU_OK; ++attempt) {
        const std::string pch = spec_pch(include_dir, cache_dir, options, g_pch_beside_refused);
        if (pch.empty()) break;
        std::vector<std::string> with = options;
        with.push_back("-include-pch");
        with.push_back(pch);
        if ((rc = compile_specialised(src, with, groups, img))) {
            // (whatever it was: the plain build below tells.)  The header beside the library may have been made under other
            // paths (a copied installation): then this process makes its own in the cache directory; one of the cache
            // directory that this compiler refuses goes, so that the next process makes a new one.
            const bool in_dir = cache_dir && *cache_dir && pch.compare(0, std::strlen(cache_dir), cache_dir) == 0;
            if (in_dir) {
                g_pch_refused = true;
                (void)std::remove(pch.c_str());
            } else {
                g_pch_beside_refused = true;
            }
        }
    }
    if (rc != HU_OK && (rc = compile_specialised(src, options, groups, img))) return rc;
    if (cached) {
        spec_cache_store(cache_dir, path, key, img);
        spec_cache_prune(cache_dir);
    }
    return HU_OK;
}

// Load `img` (the kernels of `set`) into the tape: those of them that are still missing take their slots.
int load_specialised(hu_tape t, const SpecImage& img, uint32_t set, hipError_t* why)
{
    hipModule_t module = nullptr;
    hipFunction_t loaded[kSpecKernelCount] = {};
    hipError_t e = hipModuleLoadData(&module, img.code.data());
    size_t next = 0;
    for (int i = 0; i < kSpecKernelCount && e == hipSuccess; ++i)
        if (kSpecGroupOf[i] & set) e = (next < img.lowered.size()) ? hipModuleGetFunction(&loaded[i], module, img.lowered[next++].c_str()) : hipErrorNotFound;
    if (e != hipSuccess) {
        if (module) (void)hipModuleUnload(module);
        (void)hipGetLastError();  // the failed load must not surface at the next launch's error check
        if (why) *why = e;
        return HU_ERR_HIP;
    }
    if (!t->spec) t->spec = new SpecKernels();
    SpecKernels* k = t->spec;
    hipFunction_t* slots[kSpecKernelCount] = {&k->dense[0], &k->dense[1], &k->blocks[0], &k->blocks[1],
                                              &k->classify[0][0], &k->classify[0][1], &k->classify[1][0], &k->classify[1][1],
                                              &k->ray_caster, &k->bitmap, &k->box_masks,
                                              &k->dense_ragged[0], &k->dense_ragged[1], &k->blocks_ragged[0], &k->blocks_ragged[1],
                                              &k->dense_runs[0], &k->dense_runs[1], &k->blocks_runs[0], &k->blocks_runs[1]};
    const uint32_t missing = set & ~k->groups;
    for (int i = 0; i < kSpecKernelCount; ++i)
        if (kSpecGroupOf[i] & missing) *slots[i] = loaded[i];
    k->modules.push_back(module);
    k->groups |= missing;
    const sdf::SpecMeta& meta = t->spec_meta;
    k->deferred = meta.deferred;
    k->coord_limit = meta.coord_limit;
    k->prune_words = meta.prune_words;
    k->prune_bits = meta.prune_bits;
    k->prune_all = meta.prune_all;
    std::memcpy(k->tabs, meta.tabs, sizeof k->tabs);
    std::memcpy(k->dtabs, meta.dtabs, sizeof k->dtabs);
    return HU_OK;
}

}  // namespace

extern "C" {

int hu_tape_compile_cached(const float* tape, size_t n, const char* include_dir, const char* cache_dir, size_t* code_bytes,
                           int* from_cache)
{
    return hu_tape_compile_groups(tape, n, include_dir, cache_dir, HU_SPEC_ALL, code_bytes, from_cache);
}

int hu_tape_compile_groups(const float* tape, size_t n, const char* include_dir, const char* cache_dir, uint32_t groups,
                           size_t* code_bytes, int* from_cache)
{
    if (!tape || !include_dir) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (groups == 0 || (groups & ~(uint32_t)HU_SPEC_ALL)) return hu_fail(HU_ERR_BAD_ARG, "groups must be a non-empty set of HU_SPEC_* bits");
    sdf::DecodedTape d;
    const std::string err = sdf::decode_tape(tape, n, d);
    if (!err.empty()) return hu_fail(HU_ERR_BAD_TAPE, "malformed tape: " + err);
    hu_tape_s t;  // host fields only
    t.n_slots = d.n_slots;
    keep_programs(&t, d);
    SpecImage img;
    int rc;
    if ((rc = specialised_image(generate_source(&t), include_dir, cache_dir, false, groups, img, from_cache))) return rc;
    if (code_bytes) *code_bytes = img.code.size();
    return HU_OK;
}

int hu_spec_pch_prepare(const char* include_dir, const char* dir, char* path, size_t capacity)
{
    if (!include_dir || !dir) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    // one per set of options the builds use: small sources (-O3) and big ones (-O1): clang refuses a header made at another level
    const std::string pch = spec_pch(include_dir, dir, spec_options(include_dir, false), true);
    const std::string pch_big = spec_pch(include_dir, dir, spec_options(include_dir, true), true);
    if (path && capacity) std::snprintf(path, capacity, "%s%s%s", pch.c_str(), (pch.empty() || pch_big.empty()) ? "" : "\n", pch_big.c_str());
    return HU_OK;
}

int hu_tape_compile_check(const float* tape, size_t n, const char* include_dir, size_t* code_bytes)
{
    return hu_tape_compile_cached(tape, n, include_dir, nullptr, code_bytes, nullptr);
}

int hu_tape_specialize_cached(hu_tape t, const char* include_dir, const char* cache_dir, int only_if_cached, int* from_cache)
{
    return hu_tape_specialize_groups(t, include_dir, cache_dir, only_if_cached, HU_SPEC_ALL, from_cache);
}

int hu_tape_specialize_groups(hu_tape t, const char* include_dir, const char* cache_dir, int only_if_cached, uint32_t groups, int* from_cache)
{
    if (from_cache) *from_cache = 0;
    if (!t || !include_dir) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (groups & ~(uint32_t)HU_SPEC_ALL) return hu_fail(HU_ERR_BAD_ARG, "groups must be a set of HU_SPEC_* bits");
    auto missing = [&] { return t->spec ? (groups & ~t->spec->groups) : groups; };   // kernels that are loaded stay as they are
    if (missing() == 0) return HU_OK;
    if (t->spec_source.empty()) t->spec_source = generate_source(t, &t->spec_meta);
    const std::string& src = t->spec_source;
    const bool cache = cache_dir && *cache_dir;
    bool all_cached = true;
    // 1. the image of exactly this set (what a synchronous build of it left in the cache), 2. the images of its single
    // kernels (what the background builds leave), both only read; 3. what is still missing, built as one image
    for (int step = 0; step < 3 && missing(); ++step) {
        if (step < 2 && !cache) continue;
        if (step == 2 && only_if_cached) break;
        std::vector<uint32_t> sets;
        if (step == 1) {
            for (int i = 0; i < kSpecKernelCount; ++i)
                if ((kSpecGroupOf[i] & missing()) && kSpecGroupOf[i] != groups) sets.push_back(kSpecGroupOf[i]);
        } else {
            sets.push_back(step == 0 ? groups : missing());
        }
        for (uint32_t set : sets) {
            for (int attempt = 0; attempt < 2; ++attempt) {
                SpecImage img;
                int crc, cached = 0;
                // second attempt (step 3 only): the cached image did not load (e.g. written by an incompatible runtime): build and replace it
                if ((crc = specialised_image(src, include_dir, cache_dir, step < 2, set, img, &cached, attempt != 0))) return crc;
                if (img.code.empty()) break;  // not cached: still interpreted
                hipError_t e = hipSuccess;
                if (load_specialised(t, img, set, &e) == HU_OK) {
                    all_cached = all_cached && cached;
                    break;
                }
                if (step < 2) break;       // an unusable cached image is not the caller's problem
                if (!cached || attempt == 1) return hu_fail(HU_ERR_HIP, std::string("loading the specialised module: ") + hipGetErrorString(e));
            }
        }
    }
    if (from_cache) *from_cache = (all_cached && missing() == 0) ? 1 : 0;
    return HU_OK;
}

int hu_tape_specialize(hu_tape t, const char* include_dir) { return hu_tape_specialize_cached(t, include_dir, nullptr, 0, nullptr); }

int hu_tape_source(const float* tape, size_t n, char* buf, size_t capacity, size_t* needed)
{
    if (!tape || !needed || (!buf && capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    sdf::DecodedTape d;
    const std::string err = sdf::decode_tape(tape, n, d);
    if (!err.empty()) return hu_fail(HU_ERR_BAD_TAPE, "malformed tape: " + err);
    hu_tape_s t;  // host fields only: nothing touches a device
    t.n_slots = d.n_slots;
    keep_programs(&t, d);
    const std::string src = generate_source(&t);
    *needed = src.size() + 1;
    if (capacity >= src.size() + 1) std::memcpy(buf, src.c_str(), src.size() + 1);
    return HU_OK;
}

int hu_tape_listing(const float* tape, size_t n, int which, char* buf, size_t capacity, size_t* needed)
{
    if (!tape || !needed || (!buf && capacity)) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    if (which < 0 || which > 3) return hu_fail(HU_ERR_BAD_ARG, "which must be 0..3");
    sdf::DecodedTape d;
    const std::string err = sdf::decode_tape(tape, n, d);
    if (!err.empty()) return hu_fail(HU_ERR_BAD_TAPE, "malformed tape: " + err);
    const std::vector<Rec>& prog = which == 0 ? d.recs : which == 1 ? d.recs_do : which == 2 ? d.fused : d.fused_do;
    static const char* const internal[] = {"FROM_SCALE", "FROM_X", "FROM_Y", "FROM_Z", "POINT", "TO_SCALE", "TO_X", "TO_Y", "TO_Z",
                                           "TO_ROW_X", "TO_ROWS_YZ", "FROM_MATRIX", "INIT_ROW_X", "INIT_ROWS_YZ", "LEAF"};
    static const char* const kinds[] = {"-", "scale", "x", "y", "z"};
    static const char* const prims[] = {"rectangle", "circle", "sphere", "half_space"};
    static const char* const combs[] = {"", "union", "intersection", "subtraction"};
    std::ostringstream o;
    for (const Rec& r : prog) {
        const uint32_t op = r.hdr & 0xffu, slot = (r.hdr >> 8) & 0xffffu;
        uint32_t fold;
        std::memcpy(&fold, &r.p[sdf::kFoldParam], 4);
        if (fold & sdf::kFoldLoad) o << "[load " << (fold & 0xffu) << ((fold & sdf::kFoldLoadResult) ? "r" : "") << "] ";
        o << (op < sdf::OP_COUNT ? sdf::op_info(op).name : internal[op - sdf::OP_COUNT]);
        if (op == sdf::OPX_LEAF) {
            uint32_t c;
            std::memcpy(&c, &r.p[sdf::kLeafControl], 4);
            o << "(" << ((c & sdf::kLeafSample) ? "sample " : "") << "to:" << kinds[(c >> sdf::kLeafToShift) & 7u]
              << ((c & sdf::kLeafMidStore) ? " store-point:" + std::to_string(slot) : std::string()) << " "
              << prims[(c >> sdf::kLeafPrimShift) & 3u] << ((c & sdf::kLeafExtrusion) ? " extrusion" : "")
              << " from:" << kinds[(c >> sdf::kLeafFromShift) & 7u];
            for (int k = 0; k < 2; ++k) {
                const uint32_t cb = c >> (k == 0 ? sdf::kLeafComb1Shift : sdf::kLeafComb2Shift);
                if (cb & 3u) o << " " << combs[cb & 3u] << ":" << ((cb >> 2) & 0xffu);
            }
            o << ")";
        } else if (sdf::rec_arity(op) == 2 || op == sdf::OP_STORE || op == sdf::OP_LOAD) {
            o << " " << slot << ((r.hdr & sdf::kResultKind) ? "r" : "");
        }
        if (fold & sdf::kFoldStore) o << " [store " << ((fold >> 16) & 0xffu) << ((fold & sdf::kFoldStoreResult) ? "r" : "") << "]";
        o << "\n";
        if (op == sdf::OP_RETURN) break;
    }
    const std::string text = o.str();
    *needed = text.size() + 1;
    if (capacity >= text.size() + 1) std::memcpy(buf, text.c_str(), text.size() + 1);
    return HU_OK;
}

int hu_tape_coordinate_limit(const float* tape, size_t n, double* out_limit)
{
    if (!tape || !out_limit) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    sdf::DecodedTape d;
    const std::string err = sdf::decode_tape(tape, n, d);
    if (!err.empty()) return hu_fail(HU_ERR_BAD_TAPE, "malformed tape: " + err);
    hu_tape_s t;  // host fields only: nothing touches a device
    t.n_slots = d.n_slots;
    keep_programs(&t, d);
    sdf::SpecMeta meta;   // (what hu_tape_specialize keeps beside the source, and load_specialised hands to the launches)
    (void)generate_source(&t, &meta);
    *out_limit = meta.coord_limit;
    return HU_OK;
}

int hu_tape_prune_info(hu_tape t, int* bits, int* words)
{
    if (!t) return hu_fail(HU_ERR_BAD_ARG, "tape is NULL");
    if (bits) *bits = t->spec ? t->spec->prune_bits : 0;
    if (words) *words = t->spec ? t->spec->prune_words : 0;
    return HU_OK;
}

int hu_tape_specialized(hu_tape t, int* out)
{
    if (!t || !out) return hu_fail(HU_ERR_BAD_ARG, "NULL argument");
    *out = t->spec ? (int)t->spec->groups : 0;   // the HU_SPEC_* families that are loaded (0: interpreted)
    return HU_OK;
}

}  // extern "C"
