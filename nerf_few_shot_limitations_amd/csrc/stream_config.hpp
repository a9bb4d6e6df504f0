// stream_config.hpp -- geometry of the packed weight stream, shared by the host packer and the kernels
#pragma once

namespace nrf {

constexpr int kChunkFrags = 16;     // 1-KiB fragments per chunk (one barrier per chunk)
constexpr int kSlots = 6;           // LDS ring depth in chunks (kChunkFrags * kSlots KiB); 6 and 8 measure the same (profiles/README.md)

}  // namespace nrf
