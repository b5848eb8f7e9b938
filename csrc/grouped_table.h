// grouped_table.h — layout of the descriptor table of a grouped ragged launch
// (ft_ragged.hpp, GROUPED), shared by host and device.  The table is one
// device allocation of grouped_table_bytes(groups) bytes that the host fills
// (grouped_table_build, dispatch.hip) and the caller uploads:
//
//   int tile_start[groups + 1]   exclusive prefix of the entries' tile counts
//                                ceil(M/BM) * ceil(N/BN); the last is the grid
//   (padding to 16 bytes)
//   GroupedEntry entry[groups]
//
// An entry with M == 0 or N == 0 has no tiles: its tile_start equals its
// successor's and no block ever loads its descriptor.  A stream-K launch
// appends one more section (GroupSkTable, below).
#pragma once

#include <cstddef>

namespace ftsgemm {

// What the prologue of a grouped block loads.  Pointers are the entry's own;
// `fast` holds the RaggedFast bits the leading dimensions allow (the kernel
// clears those the pointers do not); wstride is the verify / inject window
// stride in panels of this entry's K; ws_off is where the entry's segment
// sums start in the launch's workspace, in floats, rows sstr pairs long.
struct GroupedEntry {
  const float* A;
  const float* B;
  float* C;
  long long ws_off;
  int M, N, K;
  int lda, ldb, ldc;
  int fast, wstride, sstr;
  int tiles_x;  // ceil(M / BM): block t of the entry is (t % tiles_x, t / tiles_x)
};

// The table as the kernels take it (by value; built from the one device
// pointer by grouped_table_view).  A default-constructed one is "no table".
struct GroupTable {
  const int* tile_start = nullptr;
  const GroupedEntry* entry = nullptr;
  int groups = 0;
};

inline size_t grouped_prefix_bytes(int groups) {
  return (((size_t)groups + 1) * sizeof(int) + 15) & ~(size_t)15;
}

inline size_t grouped_table_bytes(int groups) {
  return groups < 0 ? 0
                    : grouped_prefix_bytes(groups) +
                          (size_t)groups * sizeof(GroupedEntry);
}

inline GroupTable grouped_table_view(const void* table, int groups) {
  const char* p = (const char*)table;
  return {(const int*)p, (const GroupedEntry*)(p + grouped_prefix_bytes(groups)),
          groups};
}

// The stream-K section of a table (ft_ragged_grouped_streamk.hpp), appended
// behind the entries so that what the classic grouped kernels read keeps its
// place and meaning.  A table built with GroupedArgs::sk_grid > 0 is
// grouped_streamk_table_bytes(groups) bytes long:
//
//   (the classic table, padded to 16 bytes)
//   int unit_start[groups + 1]   exclusive prefix of the entries' work units
//                                tiles_e * max(1, ceil(K_e / 64)); the last
//                                is the launch's unit count
//   (padding to 16 bytes)
//   int istride[groups]          verify / inject stride of entry e in 64-k
//                                units: window_stride(upt_e, verify_windows)
struct GroupSkTable {
  const int* unit_start = nullptr;
  const int* istride = nullptr;
};

inline size_t grouped_sk_section_offset(int groups) {
  return (grouped_table_bytes(groups) + 15) & ~(size_t)15;
}

inline size_t grouped_streamk_table_bytes(int groups) {
  return groups < 0 ? 0
                    : grouped_sk_section_offset(groups) +
                          grouped_prefix_bytes(groups) +
                          (size_t)groups * sizeof(int);
}

inline GroupSkTable grouped_sk_table_view(const void* table, int groups) {
  const char* p = (const char*)table + grouped_sk_section_offset(groups);
  return {(const int*)p, (const int*)(p + grouped_prefix_bytes(groups))};
}

}  // namespace ftsgemm
