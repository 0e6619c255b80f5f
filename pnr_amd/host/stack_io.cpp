// stack_io.cpp -- save_stack_u8 (stack_io.h): a multi-page uncompressed 8-bit TIFF, or bare bytes for .raw, written atomically.
#include "stack_io.h"
#include <cstdio>
#include <cstring>
#include <vector>
#include <unistd.h>

namespace advantra {

namespace {
constexpr int TAGS = 9;                               // ImageWidth .. StripByteCounts below
constexpr long long IFD_BYTES = 2 + 12 * TAGS + 4;    // count, entries, the offset of the next directory
constexpr long long TIFF_LIMIT = 0xffffffffll;        // classic TIFF: every offset is 32 bits

void put16(std::vector<unsigned char> &b, unsigned v) { b.push_back((unsigned char)(v & 255)), b.push_back((unsigned char)(v >> 8 & 255)); }
void put32(std::vector<unsigned char> &b, unsigned long v)
{
    for (int k = 0; k < 4; k++) b.push_back((unsigned char)(v >> (8 * k) & 255));
}
void entry(std::vector<unsigned char> &b, unsigned tag, unsigned type, unsigned long value)
{
    put16(b, tag), put16(b, type), put32(b, 1);
    if (type == 3) put16(b, (unsigned)value), put16(b, 0);
    else put32(b, value);
}
} // namespace

long long tiff_u8_bytes(long long w, long long h, long long l)
{
    if (w < 1 || h < 1 || l < 1 || w > TIFF_LIMIT || h > TIFF_LIMIT || l > TIFF_LIMIT) return -1;
    if (w > TIFF_LIMIT / h || w * h > TIFF_LIMIT / l) return -1;
    const long long pixels = w * h * l, total = 8 + pixels + (pixels & 1) + l * IFD_BYTES;
    return total > TIFF_LIMIT ? -1 : total;
}

bool save_stack_u8(const std::string &path, const unsigned char *data, long long w, long long h, long long l, std::string &err)
{
    if (w < 1 || h < 1 || l < 1) { err = "save_stack_u8: empty stack"; return false; }
    const bool raw = path.size() > 4 && path.substr(path.size() - 4) == ".raw";
    if (!raw && tiff_u8_bytes(w, h, l) < 0) {
        err = "cannot write " + path + ": " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(l) +
              " voxels pass the 4 GiB limit of classic TIFF (BigTIFF is not written): use a .raw name";
        return false;
    }
    const size_t pixels = (size_t)(w * h * l);
    const std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) { err = "cannot create " + tmp; return false; }
    bool ok = true;
    if (raw) ok = fwrite(data, 1, pixels, f) == pixels;
    else {
        // header | the pages' pixels | (a pad byte) | one directory per page
        const unsigned long first = (unsigned long)(8 + pixels + (pixels & 1));
        std::vector<unsigned char> head = {'I', 'I', 42, 0};
        put32(head, first);
        ok = fwrite(head.data(), 1, head.size(), f) == head.size() && fwrite(data, 1, pixels, f) == pixels;
        std::vector<unsigned char> dir;
        dir.reserve((size_t)(l * IFD_BYTES) + 1);
        if (pixels & 1) dir.push_back(0);
        for (long long z = 0; z < l; z++) {
            put16(dir, TAGS);
            entry(dir, 256, 4, (unsigned long)w);                   // ImageWidth
            entry(dir, 257, 4, (unsigned long)h);                   // ImageLength
            entry(dir, 258, 3, 8);                                  // BitsPerSample
            entry(dir, 259, 3, 1);                                  // Compression: none
            entry(dir, 262, 3, 1);                                  // PhotometricInterpretation: black is zero
            entry(dir, 273, 4, (unsigned long)(8 + z * w * h));     // StripOffsets: the page is one strip
            entry(dir, 277, 3, 1);                                  // SamplesPerPixel
            entry(dir, 278, 4, (unsigned long)h);                   // RowsPerStrip
            entry(dir, 279, 4, (unsigned long)(w * h));             // StripByteCounts
            put32(dir, z + 1 < l ? first + (unsigned long)((z + 1) * IFD_BYTES) : 0);
        }
        ok = ok && fwrite(dir.data(), 1, dir.size(), f) == dir.size();
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) {
        (void)remove(tmp.c_str());
        err = "cannot write " + path;
        return false;
    }
    return true;
}

} // namespace advantra
