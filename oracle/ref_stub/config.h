/* TEST SCAFFOLDING ONLY: the reference's cityhash/city.cc includes the
 * autoconf-generated "config.h".  Empty on purpose: little-endian host (no
 * WORDS_BIGENDIAN), no HAVE_BUILTIN_EXPECT. */
