// stack_io.h -- the host's volume writer: what --mask / --residual write and load_stack / --info read back.  No GPU, no HIP headers.
#pragma once
#include <cstdint>
#include <string>

namespace advantra {

// the bytes a classic TIFF of w x h x l 8-bit voxels takes (header, pixel data, one directory per page); -1 when it would pass 4 GiB
long long tiff_u8_bytes(long long w, long long h, long long l);
// data (w*h*l bytes, x fastest: i = z*w*h + y*w + x) as a multi-page uncompressed 8-bit grey TIFF (little-endian, one strip per page), or
// the bare bytes when the name ends in .raw.  The file is written under a temporary name beside `path` and renamed, so a reader never
// sees half a stack.  A TIFF that would pass classic TIFF's 4 GiB is refused before anything is written (err names the limit; BigTIFF
// is not written).  Returns false with a message in `err`.
bool save_stack_u8(const std::string &path, const unsigned char *data, long long w, long long h, long long l, std::string &err);

} // namespace advantra
