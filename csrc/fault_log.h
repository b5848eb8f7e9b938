// fault_log.h — layout of the fused-ABFT fault log, shared by host and
// device.  The log is caller-owned device memory: an int32 counter block
// and a ring of `capacity` fixed-size event records.  Only the cold
// locate/correct path of the fused kernels (ft_kernels.hpp locate_correct)
// writes it; with no log attached (counters == nullptr) nothing is touched.
#pragma once

namespace ftsgemm {

// Counter block, int32 each.  n_events counts every event ever taken, also
// those dropped because their slot was >= capacity.
enum FaultCounter {
  FLOG_N_EVENTS = 0,    // event slots handed out (corrected + uncorrected)
  FLOG_TRIPPED = 1,     // locate_correct entries (one per tripped wave)
  FLOG_CORRECTED = 2,   // bad columns whose row was located and corrected
  FLOG_UNCORRECTED = 3, // bad columns whose row fell outside the wave tile
  FLOG_UNLOCATED = 4,   // entries in which no column exceeded tau
  FLOG_N_COUNTERS = 5
};

// Event record, FLOG_EVENT_DWORDS int32 each.  Coordinates are those of the
// tile grid.  In a ragged launch (ft_ragged.hpp) an edge tile reaches past
// the matrix, and a fault absorbed in that zero padding is corrected and
// logged like any other, with its true padded coordinates: i >= M or j >= N
// is possible there, and k_end, a whole number of panels, may exceed K.
enum FaultEventField {
  FLOG_EV_I = 0,         // global row of the faulty element, -1 if unknown
  FLOG_EV_J = 1,         // global column of the faulty element
  FLOG_EV_K_BEGIN = 2,   // verify window (or stream-K unit group) the fault
  FLOG_EV_K_END = 3,     //   was absorbed in: [k_begin, k_end)
  FLOG_EV_STATUS = 4,    // FLOG_STATUS_*
  FLOG_EV_MAGNITUDE = 5, // float bits of rc, the value (to be) subtracted
  FLOG_EV_BAND_ROW = 6,  // first global row of the wave tile
  FLOG_EV_BAND_ROWS = 7, // rows of the wave tile (FM * MM)
  FLOG_EVENT_DWORDS = 8
};

enum FaultStatus { FLOG_STATUS_CORRECTED = 1, FLOG_STATUS_UNCORRECTED = 2 };

// Device pointers; capacity is in records.  A default-constructed log is
// "none attached".
struct FaultLog {
  int* counters = nullptr;  // FLOG_N_COUNTERS int32
  int* events = nullptr;    // capacity * FLOG_EVENT_DWORDS int32
  int capacity = 0;
};

}  // namespace ftsgemm
