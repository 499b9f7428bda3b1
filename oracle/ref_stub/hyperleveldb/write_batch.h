// TEST SCAFFOLDING ONLY (oracle/Makefile, target _ref/libref_store.so).
// Stand-in for <hyperleveldb/write_batch.h>: named in declarations only.
#ifndef hyperleveldb_write_batch_h_
#define hyperleveldb_write_batch_h_
namespace leveldb {
class WriteBatch {};
}  // namespace leveldb
#endif
