// Memory-safety check of the JPEG host pass (spe_amd/csrc/jpeg_entropy.h), a stand-alone host program meant for a sanitizer build:
//
//   python tools/gen_jpeg_golden.py --dump-dir /tmp/jpeg_files
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o /tmp/jpeg_host_check
//   /tmp/jpeg_host_check /tmp/jpeg_files
//
// It calls probe + entropy on (1) every file whole, (2) every prefix of three of the files, (3) 2000 deterministic single-byte
// corruptions of each file.  The input of every call is a heap copy of exactly n bytes and the coefficient buffer has exactly the
// elements probe asked for, so a read or write one byte outside either is a sanitizer report.  Every call must return a status;
// whole files must return 0.  Exit status 0: all of that held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <dirent.h>
#include <map>
#include <string>
#include <vector>

#include "../spe_amd/csrc/jpeg_entropy.h"

static std::map<int, long> tally;
static const long MAX_ELEMS = 1l << 26;      // a corrupted size field may ask for gigabytes: give less and expect -2

static int run(const unsigned char* src, long n) {
    std::vector<unsigned char> data(src, src + n);                            // exactly n bytes
    std::vector<int> info(SPE_JPEG_INFO_INTS);
    int rc = spe_jpeg_probe_impl(n ? data.data() : nullptr, n, info.data());
    if (rc == 0) {
        const long want = (long)info[JI_BLOCKS] * 64, have = std::min(want, MAX_ELEMS);
        std::vector<short> coef((size_t)have);
        int reason = 0;
        rc = spe_jpeg_entropy_impl(data.data(), n, coef.data(), have, &reason);
        if (rc == -2 && have == want) { std::printf("buffer refused at its full size\n"); std::exit(2); }
    }
    if (rc != 0 && rc != -2 && rc != SPE_JPEG_UNSUPPORTED && rc != SPE_JPEG_CORRUPT) { std::printf("unknown status %d\n", rc); std::exit(2); }
    ++tally[rc];
    return rc;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: %s DIR\n", argv[0]); return 2; }
    std::vector<std::string> names;
    if (DIR* dir = opendir(argv[1])) {
        while (dirent* e = readdir(dir)) {
            const std::string s = e->d_name;
            if (s.size() > 4 && s.substr(s.size() - 4) == ".jpg") names.push_back(s);
        }
        closedir(dir);
    }
    std::sort(names.begin(), names.end());
    if (names.empty()) { std::printf("no .jpg files in %s\n", argv[1]); return 2; }
    std::vector<std::vector<unsigned char>> files;
    for (const std::string& s : names) {
        FILE* f = std::fopen((std::string(argv[1]) + "/" + s).c_str(), "rb");
        if (!f) { std::printf("cannot read %s\n", s.c_str()); return 2; }
        std::vector<unsigned char> buf;
        unsigned char chunk[4096];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
        std::fclose(f);
        files.push_back(buf);
    }
    long calls = 0;
    for (size_t i = 0; i < files.size(); ++i, ++calls)
        if (run(files[i].data(), (long)files[i].size()) != 0) { std::printf("%s: a whole file was refused\n", names[i].c_str()); return 1; }
    std::printf("whole files: %zu, all status 0\n", files.size());
    // every prefix of three files below 16 KiB: the first, the middle and the last of those, by name
    std::vector<size_t> small;
    for (size_t i = 0; i < files.size(); ++i) if (files[i].size() < 16384) small.push_back(i);
    for (size_t pick : {(size_t)0, small.size() / 2, small.size() - 1}) {
        const std::vector<unsigned char>& f = files[small[pick]];
        for (size_t k = 0; k < f.size(); ++k, ++calls) {
            const int rc = run(f.data(), (long)k);
            if (rc == 0 && k + 2 < f.size()) { std::printf("%s: prefix %zu of %zu decoded\n", names[small[pick]].c_str(), k, f.size()); return 1; }
        }
        std::printf("prefixes of %s: %zu\n", names[small[pick]].c_str(), f.size());
    }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < files.size(); ++i) {
        std::vector<unsigned char> f = files[i];
        for (int t = 0; t < 2000; ++t, ++calls) {
            rng = rng * 6364136223846793005ull + 1442695040888963407ull;
            const size_t at = (size_t)((rng >> 33) % f.size());
            const unsigned char old = f[at], val = (unsigned char)(rng >> 20);
            f[at] = val == old ? (unsigned char)~old : val;
            run(f.data(), (long)f.size());
            f[at] = old;
        }
    }
    std::printf("calls: %ld\n", calls);
    for (const auto& kv : tally) std::printf("  status %d: %ld\n", kv.first, kv.second);
    return 0;
}
