// CommandTaxScreen.h — `fpmash taxscreen` (CommandTaxScreen.h, CommandTaxScreen.cpp:39-446): the
// Kraken-style report of a pool against a sketch database with an NCBI taxonomy, [percent,
// hashes in the clade, hashes in the taxon, database hashes in the clade, database hashes in the
// taxon, rank, taxonomy ID, padded name] per taxon.
#pragma once

#include "Command.h"

namespace fpmhost {

class CommandTaxScreen : public Command {
public:
    CommandTaxScreen();
    int run() const override;
};

}  // namespace fpmhost
