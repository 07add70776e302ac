// Buffer layout of the device FLAC encoder, shared by the kernel and its launcher (ou_flac_encode.hip) and the host stage
// (ou_flac.cpp): plain arithmetic, no HIP (the constexpr functions are callable from device code).  See "output files of the CLI" in include/ouniverse.h.
//   frames : file after file, block after block, one slot of flac_slot_bytes(channels, bps) bytes per block (a multiple of 16, so
//            every slot starts on a 16-byte boundary of the buffer)
//   sizes  : one int32 per slot in the same order: the bytes of the frame in it, its two CRC-16 bytes included
//   pcm    : file after file, the interleaved little-endian samples at ceil(bps / 8) bytes each, every file rounded up to 16 bytes
#pragma once
#include <cstdint>
#include <string>

namespace ou {

constexpr int kFlacBlock = 4096;                         // samples of a block (the last one of a file may be shorter)
constexpr long long kFlacMaxLen = (1ll << 36) - 1;       // STREAMINFO counts samples in 36 bits
constexpr int kFlacHeaderMax = 16;                       // sync 2, codes 2, frame number <= 7, block size 2, CRC-8 1 = 14, rounded

constexpr long long flac_blocks(long long len) { return (len + kFlacBlock - 1) / kFlacBlock; }
// the longest frame of a block: header, `channels` verbatim subframes (never shorter ones: the encoder falls back), CRC-16
constexpr long long flac_frame_max(int channels, int bps) {
  return kFlacHeaderMax + ((long long)channels * (8 + (long long)kFlacBlock * bps) + 7) / 8 + 2;
}
constexpr long long flac_slot_bytes(int channels, int bps) { return (flac_frame_max(channels, bps) + 15) & ~15ll; }
constexpr long long flac_pcm_bytes(int channels, long long len, int bps) {
  return ((long long)channels * len * ((bps + 7) / 8) + 15) & ~15ll;
}

// "" when the arguments can be encoded, the refusal otherwise
inline std::string flac_shape_error(int files, const int32_t* channels, const int64_t* len, int bps) {
  if (files < 1) return "files must be at least 1";
  if (!channels || !len) return "null argument";
  if (bps != 16 && bps != 24) return "bits per sample must be 16 or 24, got " + std::to_string(bps);
  for (int f = 0; f < files; f++) {
    if (channels[f] < 1 || channels[f] > 8)
      return "channels[" + std::to_string(f) + "] = " + std::to_string(channels[f]) + ": 1 to 8 channels";
    if (len[f] < 1 || len[f] > kFlacMaxLen)
      return "len[" + std::to_string(f) + "] = " + std::to_string((long long)len[f]) + ": 1 to 2^36 - 1 samples";
  }
  return "";
}

struct FlacTotals {
  long long frames = 0, frames_bytes = 0, pcm_bytes = 0, rows = 0;
};
// sums over all files (the arguments have passed flac_shape_error); false when a sum leaves 2^62
inline bool flac_totals(int files, const int32_t* channels, const int64_t* len, int bps, FlacTotals& t) {
  constexpr long long kMax = 1ll << 62;
  for (int f = 0; f < files; f++) {
    const long long nb = flac_blocks(len[f]), slot = flac_slot_bytes(channels[f], bps);
    const long long pcm = flac_pcm_bytes(channels[f], len[f], bps);
    if (nb > (kMax - t.frames_bytes) / slot || pcm > kMax - t.pcm_bytes) return false;
    t.frames += nb;
    t.frames_bytes += nb * slot;
    t.pcm_bytes += pcm;
    t.rows += channels[f];
  }
  return true;
}

// the message of ou_flac_last_error (ou_flac.cpp); returns `code`
int flac_fail(int code, const std::string& msg);

}  // namespace ou
