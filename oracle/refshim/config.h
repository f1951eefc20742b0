// refshim/config.h -- the build-configuration header the blocks under test include under HAVE_CONFIG_H; empty here.
#pragma once
