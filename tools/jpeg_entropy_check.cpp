// Runs the host stage of the JPEG decoder (locov_amd/csrc/jpeg_entropy.h) over every file of a directory: parse, decode, pack.
// A stand-alone program for the sanitizers (tests/test_jpeg_entropy_sanitized.py):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_entropy_check.cpp -o check
//     ./check DIR
// The staging and record buffers are malloc'ed at exactly the sizes the header asks for, so a write past either is a report.  One
// line per file: "<name> supported=<0|1> reason=<n> status=<n> record_bytes=<n> sum=<fnv of the record>".  All files are decoded a
// second time in one batched call (the threads), and the statuses must agree.  Exit status 0 unless a file cannot be read or the
// two passes disagree.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../locov_amd/csrc/jpeg_entropy.h"

using namespace locov::jpeg;

static bool read_file(const std::string &path, std::vector<uint8_t> &out)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[4096];
    size_t got;
    out.clear();
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
    std::fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 2;
    }
    DIR *dir = opendir(argv[1]);
    if (!dir) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<std::string> names;
    while (dirent *e = readdir(dir))
        if (e->d_name[0] != '.') names.push_back(e->d_name);
    closedir(dir);
    std::sort(names.begin(), names.end());

    const int n = (int)names.size();
    std::vector<uint8_t *> data(n, nullptr);                      // exact-size copies: a read past the end is a report
    std::vector<int64_t> lens(n, 0);
    std::vector<locov_jpeg_header> headers(n);
    std::vector<int> status(n, 0);
    for (int i = 0; i < n; i++) {
        std::vector<uint8_t> bytes;
        if (!read_file(std::string(argv[1]) + "/" + names[i], bytes)) {
            std::fprintf(stderr, "cannot read %s\n", names[i].c_str());
            return 2;
        }
        lens[i] = (int64_t)bytes.size();
        data[i] = static_cast<uint8_t *>(std::malloc(bytes.size() ? bytes.size() : 1));
        if (!bytes.empty()) std::memcpy(data[i], bytes.data(), bytes.size());
        parse(data[i], lens[i], &headers[i]);
        const int64_t need = entropy_bytes(headers[i], lens[i]);
        void *staging = std::malloc(need ? (size_t)need : 4);
        int64_t record_bytes = 0;
        status[i] = decode_scan(data[i], lens[i], headers[i], staging, need, &record_bytes);
        uint32_t sum = 2166136261u;
        if (status[i] == LOCOV_JPEG_STATUS_OK) {
            uint8_t *record = static_cast<uint8_t *>(std::malloc((size_t)record_bytes));
            if (!pack_record(headers[i], staging, record_bytes, record)) {
                std::fprintf(stderr, "%s: pack_record refused what decode_scan wrote\n", names[i].c_str());
                return 1;
            }
            for (int64_t k = 0; k < record_bytes; k++) sum = (sum ^ record[k]) * 16777619u;
            std::free(record);
        }
        std::free(staging);
        std::printf("%s supported=%d reason=%d status=%d record_bytes=%lld sum=%08x\n", names[i].c_str(), headers[i].supported,
                    headers[i].reason, status[i], (long long)record_bytes, sum);
    }
    // the same streams again, on the threads of a batched call
    std::vector<void *> staging(n, nullptr);
    std::vector<int64_t> need(n, 0), record_bytes(n, 0);
    std::vector<int> again(n, 0);
    for (int i = 0; i < n; i++) {
        need[i] = entropy_bytes(headers[i], lens[i]);
        staging[i] = std::malloc(need[i] ? (size_t)need[i] : 4);
    }
    parallel_for(n, [&](int i) { again[i] = decode_scan(data[i], lens[i], headers[i], staging[i], need[i], &record_bytes[i]); });
    int bad = 0;
    for (int i = 0; i < n; i++) {
        if (again[i] != status[i]) {
            std::fprintf(stderr, "%s: status %d alone, %d in the batch\n", names[i].c_str(), status[i], again[i]);
            bad = 1;
        }
        std::free(staging[i]);
        std::free(data[i]);
    }
    return bad;
}
