// scan_reader_harness.cpp -- the host-side scan reader (toothgroupnetwork_amd/csrc/meshio.hip) as a plain CPU program, to be built
// with a sanitizer (tests/host/Makefile: address + undefined, and thread) and run over the corpus that
// `python tests/scan_reader_cases.py --dump DIR` writes.  Host code only: no GPU call, no Python, not part of pytest.
//
//   scan_reader_harness DIR              every NAME.obj + NAME.json pair: tgn_obj_count, then tgn_obj_read into heap buffers of
//                                        EXACTLY the counted size (a one-element overrun is a heap-buffer-overflow), tgn_vertex_normals
//                                        on what was read, tgn_scan_open / tgn_scan_take into exactly-sized buffers; every NAME.mesh:
//                                        tgn_vertex_normals.
//   scan_reader_harness DIR --threads 8  a serial pass over the pairs, then 8 threads over the same pairs in shuffled orders while one
//                                        more calls tgn_scan_pool_trim in a loop: every status and every row must equal the serial pass.
// Exit status 0: every call kept its contract (what the sanitizer finds it reports itself and aborts).
#include <dirent.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tgn_pointops.h"

namespace tgn {
// the library's error sink (capi.hip there): formats, so that the format strings meet their arguments under the sanitizer
void set_error(const char *fmt, ...) {
    static thread_local char text[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
}
}  // namespace tgn

static const double kYMin = -36.9843781139949, kYMax = 33.15232091532151;
static long g_failures = 0;

static void fail(const std::string &name, const char *what) {
    fprintf(stderr, "FAIL %s: %s\n", name.c_str(), what);
    ++g_failures;
}

static uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}

struct ScanResult {
    int rc = -1;
    long long n = 0;
    uint64_t hash = 0;
    bool operator==(const ScanResult &o) const { return rc == o.rc && n == o.n && hash == o.hash; }
};

// tgn_scan_open + tgn_scan_take into buffers of exactly n rows
static ScanResult scan(const std::string &obj, const std::string &json, std::atomic<long> *opened, std::atomic<long> *taken) {
    ScanResult r;
    void *handle = nullptr;
    long long n = -1;
    char jaw[64];
    r.rc = tgn_scan_open(obj.c_str(), json.c_str(), kYMin, kYMax, &handle, &n, jaw, (int)sizeof jaw);
    if (r.rc != TGN_OK) {
        if (handle) r.rc = -100;      // a handle behind a failure would never be taken back
        return r;
    }
    if (opened) ++*opened;
    r.n = n;
    double *rows = (double *)malloc((size_t)n * 7 * sizeof(double));
    float *xyz = (float *)malloc((size_t)n * 3 * sizeof(float));
    if (tgn_scan_take(handle, rows, xyz) != TGN_OK) r.rc = -101;
    if (taken) ++*taken;
    r.hash = fnv(jaw, strlen(jaw), fnv(xyz, (size_t)n * 3 * sizeof(float), fnv(rows, (size_t)n * 7 * sizeof(double))));
    free(rows);
    free(xyz);
    return r;
}

static void normals(const std::string &name, const double *v, long long nv, const long long *t, long long nf) {
    double *out = (double *)malloc((size_t)nv * 3 * sizeof(double));
    const int rc = tgn_vertex_normals(v, nv, t, nf, out);
    if (rc != TGN_OK && rc != TGN_ERR_INVALID_ARGUMENT) fail(name, "tgn_vertex_normals: unexpected status");
    if (rc == TGN_OK) fnv(out, (size_t)nv * 3 * sizeof(double));      // every element is read
    free(out);
}

static void one_obj(const std::string &name, const std::string &path, long counts[4]) {
    long long nv = -1, nf = -1;
    const int rc = tgn_obj_count(path.c_str(), &nv, &nf);
    ++counts[rc >= 0 && rc <= 3 ? rc : 2];
    if (rc != TGN_OK) {
        if (rc != TGN_ERR_INVALID_ARGUMENT && rc != TGN_ERR_UNSUPPORTED) fail(name, "tgn_obj_count: unexpected status");
        return;
    }
    double *v = (double *)malloc((size_t)nv * 3 * sizeof(double));
    long long *f = (long long *)malloc((size_t)nf * 3 * sizeof(long long));
    long long rv = -1, rf = -1;
    if (tgn_obj_read(path.c_str(), v, f, nv, nf, &rv, &rf) != TGN_OK || rv != nv || rf != nf) {
        fail(name, "tgn_obj_read does not deliver what tgn_obj_count reported");
    } else {
        for (long long i = 0; i < nf * 3; ++i) f[i] -= 1;
        normals(name, v, nv, f, nf);
    }
    free(v);
    free(f);
}

static void one_mesh(const std::string &name, const std::string &path) {
    FILE *st = fopen(path.c_str(), "rb");
    long long head[2] = {0, 0};
    if (!st || fread(head, sizeof head, 1, st) != 1) {
        fail(name, "unreadable mesh file");
        if (st) fclose(st);
        return;
    }
    const long long nv = head[0], nf = head[1];
    double *v = (double *)malloc((size_t)nv * 3 * sizeof(double));
    long long *t = (long long *)malloc((size_t)nf * 3 * sizeof(long long));
    if (fread(v, sizeof(double), (size_t)nv * 3, st) != (size_t)nv * 3 || fread(t, sizeof(long long), (size_t)nf * 3, st) != (size_t)nf * 3)
        fail(name, "short mesh file");
    else
        normals(name, v, nv, t, nf);
    fclose(st);
    free(v);
    free(t);
}

static bool ends_with(const std::string &s, const char *tail) {
    const size_t n = strlen(tail);
    return s.size() >= n && !s.compare(s.size() - n, n, tail);
}

int main(int argc, char **argv) {
    if (argc != 2 && !(argc == 4 && !strcmp(argv[2], "--threads") && atoi(argv[3]) > 0)) {
        fprintf(stderr, "usage: %s DIR [--threads N]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int n_threads = argc == 4 ? atoi(argv[3]) : 0;
    std::vector<std::string> pairs, meshes;
    DIR *d = opendir(dir.c_str());
    if (!d) {
        fprintf(stderr, "cannot open %s\n", dir.c_str());
        return 2;
    }
    while (const dirent *e = readdir(d)) {
        const std::string name = e->d_name;
        if (ends_with(name, ".obj")) pairs.push_back(name.substr(0, name.size() - 4));
        if (ends_with(name, ".mesh")) meshes.push_back(name);
    }
    closedir(d);
    std::sort(pairs.begin(), pairs.end());
    std::sort(meshes.begin(), meshes.end());
    auto obj_of = [&](const std::string &stem) { return dir + "/" + stem + ".obj"; };
    auto json_of = [&](const std::string &stem) { return dir + "/" + stem + ".json"; };

    std::atomic<long> opened{0}, taken{0};
    std::vector<ScanResult> serial(pairs.size());
    long by_status[4] = {0, 0, 0, 0}, scan_status[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < pairs.size(); ++i) {
        if (!n_threads) one_obj(pairs[i], obj_of(pairs[i]), by_status);
        serial[i] = scan(obj_of(pairs[i]), json_of(pairs[i]), &opened, &taken);
        if (serial[i].rc < 0 || serial[i].rc > 3 || serial[i].rc == TGN_ERR_LAUNCH) fail(pairs[i], "tgn_scan_open / tgn_scan_take: unexpected status");
        else ++scan_status[serial[i].rc];
    }
    if (!n_threads) {
        for (const std::string &m : meshes) one_mesh(m, dir + "/" + m);
        printf("%zu OBJ + JSON pairs, %zu meshes\n", pairs.size(), meshes.size());
        printf("tgn_obj_count / tgn_obj_read: %ld read, %ld refused (the reference raises), %ld handed back (outside the native subset)\n",
               by_status[0], by_status[1], by_status[3]);
    } else {
        std::atomic<bool> done{false};
        std::atomic<long> wrong{0}, trims{0};
        std::thread trimmer([&] {
            while (!done.load()) {
                tgn_scan_pool_trim();
                ++trims;
            }
        });
        std::vector<std::thread> workers;
        for (int k = 0; k < n_threads; ++k)
            workers.emplace_back([&, k] {
                std::vector<size_t> order(pairs.size());
                for (size_t i = 0; i < order.size(); ++i) order[i] = i;
                std::mt19937 rng(k);
                std::shuffle(order.begin(), order.end(), rng);
                for (const size_t i : order)
                    if (!(scan(obj_of(pairs[i]), json_of(pairs[i]), &opened, &taken) == serial[i])) ++wrong;
            });
        for (std::thread &w : workers) w.join();
        done = true;
        trimmer.join();
        printf("%zu OBJ + JSON pairs x %d threads, tgn_scan_pool_trim called %ld times alongside\n", pairs.size(), n_threads, trims.load());
        if (wrong) fail("threads", "a threaded result differs from the serial pass");
    }
    printf("tgn_scan_open: %ld rows, %ld refused, %ld handed back (serial pass); %ld handles opened, %ld taken back\n", scan_status[0],
           scan_status[1], scan_status[3], opened.load(), taken.load());
    if (opened != taken) fail("handles", "opened and taken counts differ");
    tgn_scan_pool_trim();
    printf(g_failures ? "%ld FAILURES\n" : "no failures\n", g_failures);
    return g_failures ? 1 : 0;
}
