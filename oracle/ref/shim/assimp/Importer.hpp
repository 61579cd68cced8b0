/* Host stand-in for <assimp/Importer.hpp>: a forward declaration only.  The
 * bridge compiles none of the reference's mesh loading. */
#ifndef PTREF_SHIM_ASSIMP_IMPORTER_HPP
#define PTREF_SHIM_ASSIMP_IMPORTER_HPP
namespace Assimp { class Importer; }
#endif
